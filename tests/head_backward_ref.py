"""Float64 references, per-element bounds and checkers for the fp32 backward kernels of the trajectory head and the small encoders
(csrc/backward.hip) -- TEST INFRASTRUCTURE ONLY; torch on the CPU, nothing here comes from a project kernel.

Every *_ref function evaluates the formula of the kernel's header once in float64 from the fp32 (fp16) input VALUES and returns,
per output, an Out(ref, f32, absum, n):
  ref    the float64 value;
  f32    the fp32 term of the realistic bound  |got - ref| <= 1.01 * f32 + ulp_out(ref), first order in E = 2^-24, built from float64
         intermediates only; a sum of terms evaluated along a chain of n roundings is charged n * E * sum |terms| (the library is
         built with -ffp-contract=off: fmaf rounds once, every other operation once), an input of the sum that already carries an
         error d is charged d on top;
  absum  the sum of the absolute values of the terms of the longest sum: below 2^24 units every partial sum, in any order, is an
         exactly representable fp32 number (integer regime: got must EQUAL ref rounded to the output type);
  n      the chain length, as read from the kernel (it goes into profiles/head_backward_bounds.txt).
The chains: a lane (thread) adds ceil(items / 64) (ceil(items / 256)) terms serially; wave_sum has 6 exchange levels; the LDS tree
of poly_embed_bwd 8; the four LDS slices of layernorm_bwd add in 3; reduce_partials adds ceil(nb / 16) rows per wave, then the 16
wave sums, then the accumulate.  rsqrtf is charged T_RSQRT = 4 E relative (the unit of the forward row tests), __expf
2 E (1 + smax): v_exp_f32 (1 ulp) of a rounded product x * log2(e) with |x| <= 2 smax -- the (1 + smax) unit with c = 2 that the
forward test charges tcavt_mha.
"""
import math

import numpy as np
import torch

from test_attention_bwd_gpu import _first_bad
from test_gemm_forms_gpu import _ulp

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
E = 2.0 ** -24
T_RSQRT = 4 * E
LN_EPS = float(np.float32(1e-5))
SEED = 20240607


class Out:
    def __init__(self, ref, f32=None, absum=None, n=0, unit=1.0, dt=F32):
        self.ref, self.n, self.unit, self.dt = ref, n, unit, dt
        self.f32 = torch.zeros_like(ref) if f32 is None else f32.expand_as(ref)
        self.absum = ref.abs() if absum is None else absum.expand_as(ref)

    def bound(self):
        return 1.01 * self.f32 + _ulp(self.ref, self.dt)

    def exact_ok(self):
        """the integer-regime precondition: every term a whole number of units, every sum of absolute values below 2^24 units"""
        r = self.ref / self.unit
        return bool((r == r.round()).all()) and self.absum.max().item() / self.unit < 2.0 ** 24

    def rounded(self):
        """ref rounded once to the output type (what a correct kernel may return at best)"""
        return self.ref.float().to(self.dt)


def check(got, out, regime, what):
    """every element of got (any device, the output type) against out; returns the worst fraction of the bound (0 if exact)"""
    g = got.detach().double().cpu().reshape(out.ref.shape)
    assert torch.isfinite(g).all(), f"{what}: {int((~torch.isfinite(g)).sum())} non-finite (unwritten?) elements in range"
    if regime == "integer":
        assert out.exact_ok(), f"{what}: the operands do not keep fp32 exact"
        bad = g != out.rounded().double()
        assert not bool(bad.any()), (f"{what}: {int(bad.sum())} elements differ; first {_first_bad(bad)}: got "
                                     f"{g[_first_bad(bad)].item()!r} ref {out.ref[_first_bad(bad)].item()!r}")
        return 0.0
    bound = out.bound()
    d = (g - out.ref).abs()
    frac = (d / bound.clamp_min(1e-300)).max().item()
    bad = d > bound
    if bool(bad.any()):
        i = _first_bad(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of bound (worst fraction {frac:.3f}); first {i}: "
                             f"got {g[i].item()!r} ref {out.ref[i].item()!r} allowed {bound[i].item():.3e}")
    return frac


# ---------------------------------------------------------------------------------------------------------------------------
# data

def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, g, r=8):
    """small integers, distinct per index: randint(-r, r) plus a per-row and a per-column offset (two swapped rows cannot cancel)"""
    t = torch.randint(-r, r + 1, shape, generator=g).double()
    rows = (torch.arange(shape[0]) % 5).double().view(-1, *([1] * (len(shape) - 1)))
    cols = 2 * (torch.arange(shape[-1]) % 3).double()
    return t + rows + (cols if len(shape) > 1 else 0)


def data(shape, regime, g, scale=1.0, r=8):
    """float64 holding fp32 values: integers (integer regime) or N(0, scale^2)"""
    if regime == "integer":
        return ints(shape, g, r)
    return (torch.randn(shape, generator=g) * scale).float().double()


def inv_keep(p):
    """1 / (1 - p) as make_dropout forms it (csrc/philox.hpp: an fp32 quotient)"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def attn_keep(B, nh, Lq, Lk, p, site, seed=SEED):
    """float64 [B, nh, Lq, Lk]: the oracle's keep mask, element ((b nh + h) Lq + i) Lk + j as mha_small_bwd_kernel states"""
    from oracle.philox import keep_mask

    return torch.from_numpy(keep_mask(B * nh * Lq * Lk, p, seed, site).astype(np.float64)).view(B, nh, Lq, Lk)


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------
# colsum, out_head_bwd, conv1x1_bwd, poly_embed_bwd, nlinear_bwd, masked_mean_bwd, mse_grad, softmax_bwd_rows

def colsum_ref(g, init=None):
    """out[n] (+)= sum_m g[m][n]: a thread adds 32 rows of its block serially, 3 additions join the four threads, a reducer wave adds
    ceil(nb / 16) partials, 16 wave sums, the accumulate"""
    M = g.shape[0]
    nb = _cdiv(M, 128)
    n = min(32, _cdiv(M, 4)) + 3 + _cdiv(nb, 16) + 16 + 1
    i0 = torch.zeros(g.shape[1], dtype=F64) if init is None else init
    A = g.abs().sum(0) + i0.abs()
    return {"out": Out(g.sum(0) + i0, n * E * A, A, n)}


def out_head_bwd_ref(g, fused, w):
    """g [B, F, To], fused [B, To, C], w [F, C].  gf: F chained fmaf.  gw, gb: a lane runs ceil(B To / 64) fmaf (additions), then
    the 6 levels of wave_sum"""
    B, F, To = g.shape
    n = _cdiv(B * To, 64) + 6
    Agf = torch.einsum("bfs,fc->bsc", g.abs(), w.abs())
    Agw = torch.einsum("bfs,bsc->fc", g.abs(), fused.abs())
    Agb = g.abs().sum((0, 2))
    return {"gf": Out(torch.einsum("bfs,fc->bsc", g, w), F * E * Agf, Agf, F),
            "gw": Out(torch.einsum("bfs,bsc->fc", g, fused), n * E * Agw, Agw, n),
            "gb": Out(g.sum((0, 2)), n * E * Agb, Agb, n)}


def conv1x1_bwd_ref(gxp, x):
    """gxp [B, T, C] token-major, x [B, F, T]: a lane runs ceil(B T / 64) fmaf (additions for gb), then wave_sum"""
    B, T, _ = gxp.shape
    n = _cdiv(B * T, 64) + 6
    Agw = torch.einsum("btc,bft->cf", gxp.abs(), x.abs())
    Agb = gxp.abs().sum((0, 1))
    return {"gw": Out(torch.einsum("btc,bft->cf", gxp, x), n * E * Agw, Agw, n), "gb": Out(gxp.sum((0, 1)), n * E * Agb, Agb, n)}


def poly_embed_bwd_ref(g, poly):
    """g [B, P, D], poly [B, P, 2]: gw, gb: a thread runs ceil(B P / 256) fmaf (additions), then the 8 levels of the LDS tree;
    gpos: B serial additions"""
    B, P, _ = g.shape
    n = _cdiv(B * P, 256) + 8
    Agw = torch.einsum("bpd,bpk->dk", g.abs(), poly.abs())
    Agb = g.abs().sum((0, 1))
    Agp = g.abs().sum(0)
    return {"gw": Out(torch.einsum("bpd,bpk->dk", g, poly), n * E * Agw, Agw, n), "gb": Out(g.sum((0, 1)), n * E * Agb, Agb, n),
            "gpos": Out(g.sum(0), B * E * Agp, Agp, B)}


def nlinear_bwd_ref(inp, W, g):
    """inp [B, T, C] token-major, W [C, S, T], g [B, C, S].  u = in - in[T-1] rounds once (E |u|).
    gW = sum_b g u: B chained fmaf on rounded u: (B + 1) E sum |g u|.  gbias: B additions.  gin[t < T-1] = sum_s g W: S chained
    fmaf, A_t = sum_s |g W|.  gin[T-1] = tot - acc: tot = sum_s g (S additions on G = sum |g|), acc = the T - 1 computed gin added
    serially (their own S E A_t each, then (T - 1) E sum_t A_t), one subtraction: E [(S + 1) G + (S + T) sum_t A_t]"""
    B, T, C = inp.shape
    S = W.shape[1]
    u = inp - inp[:, -1:, :]
    AgW = torch.einsum("bcs,btc->cst", g.abs(), u.abs())
    Agb = g.abs().sum(0)
    gin = torch.einsum("bcs,cst->btc", g, W)
    A = torch.einsum("bcs,cst->btc", g.abs(), W.abs())
    G = g.abs().sum(2)                                                            # [B, C]
    tot = g.sum(2)
    gin[:, -1, :] = tot - gin[:, :-1, :].sum(1)
    f_in = S * E * A
    f_in[:, -1, :] = E * ((S + 1) * G + (S + T) * A[:, :-1, :].sum(1))
    A_in = A.clone()
    A_in[:, -1, :] = G + A[:, :-1, :].sum(1)
    return {"gW": Out(torch.einsum("bcs,btc->cst", g, u), (B + 1) * E * AgW, AgW + inp.abs().max() * 2, B + 1),
            "gbias": Out(g.sum(0), B * E * Agb, Agb, B), "gin": Out(gin, f_in, A_in, 2 * S + T)}


def masked_mean_bwd_ref(gemb, lens, P):
    """genc[b][p][d] = p < n ? gemb[b][d] / n : 0, n = min(len[b], P): one correctly rounded fp32 division (float64's quotient
    rounded to fp32 is that value: 53 >= 2 * 24 + 2)"""
    B, D = gemb.shape
    ref = torch.zeros(B, P, D, dtype=F64)
    for b, ln in enumerate(lens):
        n = min(int(ln), P)
        if n > 0:
            ref[b, :n] = gemb[b] / n
    return {"genc": Out(ref, torch.zeros_like(ref), ref.abs(), 1)}


def mse_grad_ref(pred, gt, ns, g_loss=None, g_pred=None, unit=1.0):
    """pred, gt [B, 2, To], ns [B, 4] = (mn_x, mx_x, mn_y, mx_y).  v = 2 d r / (B To), d = (pred r + mn) - (gt r + mn), r = mx - mn.
    r rounds (E r); pred r: 2 E |pred r|; + mn: E |pred r + mn| -- the pixel-space magnitudes; the same for gt; d: E |d|; then
    r's rounding again, the product and the divide: 3 E |v|.  g_loss scales all of it and rounds once more, g_pred adds and rounds."""
    B, _, To = pred.shape
    if g_loss is None and g_pred is not None:
        return {"g": Out(g_pred.clone(), None, None, 0, unit)}
    mn, r = ns[:, [0, 2]][:, :, None], (ns[:, [1, 3]] - ns[:, [0, 2]])[:, :, None]
    pa, pb = pred * r, gt * r
    d = pa - pb
    dd = 2 * E * (pa.abs() + pb.abs()) + E * ((pa + mn).abs() + (pb + mn).abs()) + E * d.abs()
    v = 2 * d * r / (B * To)
    f = 2 * r.abs() / (B * To) * dd + 3 * E * v.abs()
    n = 8
    if g_loss is not None:
        v, f, n = v * g_loss, f * abs(g_loss) + E * (v * g_loss).abs(), n + 1
    if g_pred is not None:
        v, f, n = v + g_pred, f + E * (v + g_pred).abs(), n + 1
    return {"g": Out(v, f, v.abs() + (0 if g_pred is None else g_pred.abs()), n, unit)}


def softmax_bwd_rows_ref(P, dP, scale, n_out, unit=1.0):
    """P (fp16 values), dP [rows, n_valid].  dot = sum_c P dP: each product rounds, a lane adds ceil(n_valid / 64) of them, wave_sum:
    n = ceil(n_valid / 64) + 7 on D = sum |P dP|.  v = (scale P) (dP - dot): the difference, the two products: 3 E |v|, and
    |scale P| times dot's error.  Columns n_valid .. n_out are +0."""
    rows, nv = P.shape
    n = _cdiv(nv, 64) + 7
    dot = (P * dP).sum(1, keepdim=True)
    D = (P * dP).abs().sum(1, keepdim=True)
    v = scale * P * (dP - dot)
    ref, f = torch.zeros(rows, n_out, dtype=F64), torch.zeros(rows, n_out, dtype=F64)
    ref[:, :nv] = v
    f[:, :nv] = (scale * P).abs() * n * E * D + 3 * E * v.abs()
    A = torch.zeros(rows, n_out, dtype=F64)
    A[:, :nv] = abs(scale) * P.abs() * (dP.abs() + D)
    return {"dS": Out(ref, f, A, n + 3, unit, BF16)}


# ---------------------------------------------------------------------------------------------------------------------------
# layernorm_bwd

def layernorm_bwd_ref(x, gamma, gy, gg0, gb0, eps=LN_EPS):
    """x, gy [M, D].  With L = ceil(D / 64) and n1 = L + 6 (a lane's serial additions and wave_sum):
    mean: n1 E mean|x| + E |mean| (the divide) = dm;  d = x - mean: dd = dm + E |d| -- the cancellation term, it scales with |x|;
    var = sum d^2 / D: the products and the chain (n1 + 1) E var, the divide E var, and 2 |d| dd through the squares;  + eps: E;
    rstd = rsqrtf(.): half the relative error of its argument, and T_RSQRT;
    gg = gy gamma: E |gg|;  a = sum gg / D: (n1 + 1) E mean|gg| + E |a| = da;
    t = gg d rstd: |gg| rstd dd + |gg d| drstd + 3 E |t|;  b = sum t / D: mean(dt) + n1 E mean|t| + E |b| = db;
    xh = d rstd: dxh = rstd dd + |d| drstd + E |xh|;
    inner = gg - a - xh b: E |gg| + da + E |gg - a| + |b| dxh + |xh| db + E |xh b| + E |inner|;  gx = rstd inner: one more product.
    ggamma = start + sum_rows gy xh: a wave's 4 rows with one product each, 3 additions over the LDS slices, ceil(nb / 16) partials per
    reducer wave, 16 wave sums, the accumulate: n = 4 + 1 + 3 + ceil(nb / 16) + 16 + 1 on sum |gy xh| + |start|, and |gy| dxh;
    gbeta the same without the product."""
    M, D = x.shape
    n1 = _cdiv(D, 64) + 6
    mean = x.mean(1, keepdim=True)
    dm = n1 * E * x.abs().mean(1, keepdim=True) + E * mean.abs()
    d = x - mean
    dd = dm + E * d.abs()
    var = (d * d).mean(1, keepdim=True)
    dvar = (2 * d.abs() * dd).mean(1, keepdim=True) + (n1 + 2) * E * var
    ve = var + eps
    rstd = ve ** -0.5
    dr = rstd * (0.5 * (dvar + E * ve) / ve + T_RSQRT)
    gg = gy * gamma
    a = gg.mean(1, keepdim=True)
    da = (n1 + 1) * E * gg.abs().mean(1, keepdim=True) + E * a.abs()
    xh = d * rstd
    t = gg * xh
    dt_ = gg.abs() * rstd * dd + (gg * d).abs() * dr + 3 * E * t.abs()
    b = t.mean(1, keepdim=True)
    db = dt_.mean(1, keepdim=True) + n1 * E * t.abs().mean(1, keepdim=True) + E * b.abs()
    dxh = rstd * dd + d.abs() * dr + E * xh.abs()
    inner = gg - a - xh * b
    dinner = E * gg.abs() + da + E * (gg - a).abs() + b.abs() * dxh + xh.abs() * db + E * (xh * b).abs() + E * inner.abs()
    gx = rstd * inner
    dgx = rstd * dinner + inner.abs() * dr + E * gx.abs()
    per = _cdiv(_cdiv(M, 16), 16)
    ng, nbeta = 4 + 1 + 3 + per + 16 + 1, 4 + 3 + per + 16 + 1
    Ag = (gy * xh).abs().sum(0) + gg0.abs()
    Ab = gy.abs().sum(0) + gb0.abs()
    return {"gx": Out(gx, dgx, None, n1), "ggamma": Out(gg0 + (gy * xh).sum(0), ng * E * Ag + (gy.abs() * dxh).sum(0), Ag, ng),
            "gbeta": Out(gb0 + gy.sum(0), nbeta * E * Ab, Ab, nbeta)}


# ---------------------------------------------------------------------------------------------------------------------------
# mha_bwd

def mha_staged(Lq, Lk, dh):
    """tcavt_mha_bwd's kernel choice: q, k, v, dO staged in LDS next to P and dS when all of it fits 64 KiB"""
    return 2 * Lq * Lk * 4 + 2 * (Lq + Lk) * (dh + 1) * 4 <= 65536


def mha_bwd_ref(q, k, v, go, klen, scale, keep=None, ik=1.0, unit=1.0):
    """q, go [B, Lq, nh, dh]; k, v [B, Lk, nh, dh]; klen [B] (clamped to 0 .. Lk); keep [B, nh, Lq, Lk] or None, ik = 1 / (1 - p).
    Outputs as the kernel stores them: [B * L, nh * dh].  With S = scale sum |q k|, smax its row maximum, L = ceil(Lk / 64):
    s = scale sum q k: dh chained fmaf and the product: (dh + 1) E S;  x = s - m: E |x|, |x| <= 2 smax (the error of m itself cancels
    between numerator and denominator);  e = __expf(x): relative (dh + 3) E smax + 2 E (1 + smax);  the sum of e (L + 6), the
    reciprocal, the product:  P carries rho = 2 [(dh + 5) E smax + 2 E] + (L + 8) E relative.
    dP = sum dO v: dh chained fmaf, ddp = dh E sum |dO v|;  dropout: dP' = dP keep / (1 - p), one rounding more.
    dot = sum_j P dP': product, lane chain L, wave_sum: (L + 7) E sum |P dP'|, and sum (rho |P dP'| + P ddp').
    dS = P (dP' - dot) scale: |scale| [rho P |dP' - dot| + P (ddp' + ddot)] + 3 E |dS|.   P' = P keep / (1 - p): (rho + E) P'.
    dQ = sum_{j < klen} dS k: klen chained fmaf: sum ddS |k| + klen E sum |dS k|;  dK = sum_i dS q, dV = sum_i P' dO: Lq chained fmaf."""
    B, Lq, nh, dh = q.shape
    Lk = k.shape[1]
    L = _cdiv(Lk, 64)
    qh, kh, vh, gh = (t.permute(0, 2, 1, 3) for t in (q, k, v, go))                # [B, nh, L, dh]
    klen = torch.as_tensor(klen).long().clamp(0, Lk)
    m = (torch.arange(Lk)[None, :] < klen[:, None])[:, None, None, :]              # [B, 1, 1, Lk]
    kh, vh = kh * m.transpose(-1, -2), vh * m.transpose(-1, -2)                    # masked keys never enter a sum
    s = (qh @ kh.transpose(-1, -2)) * scale
    S = (qh.abs() @ kh.abs().transpose(-1, -2)) * abs(scale)
    smax = S.amax(-1, keepdim=True)
    sm = s.masked_fill(~m, float("-inf"))
    mx = sm.amax(-1, keepdim=True)
    e = torch.where(m, torch.exp(sm - torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))), torch.zeros_like(s))
    den = e.sum(-1, keepdim=True)
    P = torch.where(den > 0, e / den.clamp_min(1e-300), torch.zeros_like(e))
    rho = 2 * ((dh + 5) * E * smax + 2 * E) + (L + 8) * E
    kp = torch.ones_like(P) if keep is None else keep * ik
    dP = (gh @ vh.transpose(-1, -2)) * kp
    ddp = dh * E * (gh.abs() @ vh.abs().transpose(-1, -2)) * kp + (0 if keep is None else E * dP.abs())
    PdP = P * dP
    dot = PdP.sum(-1, keepdim=True)
    ddot = (rho * PdP.abs() + P * ddp).sum(-1, keepdim=True) + (L + 7) * E * PdP.abs().sum(-1, keepdim=True)
    dS = P * (dP - dot) * scale
    ddS = abs(scale) * (rho * P * (dP - dot).abs() + P * (ddp + ddot)) + 3 * E * dS.abs()
    Pp = P * kp
    dPp = (rho + E) * Pp
    kl = klen.double()[:, None, None, None]
    AQ, AK, AV = dS.abs() @ kh.abs(), dS.abs().transpose(-1, -2) @ qh.abs(), Pp.transpose(-1, -2) @ gh.abs()
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(B * t.shape[2], nh * dh)
    return {"gq": Out(flat(dS @ kh), flat(ddS @ kh.abs() + kl * E * AQ), flat(AQ), Lk, unit),
            "gk": Out(flat(dS.transpose(-1, -2) @ qh), flat(ddS.transpose(-1, -2) @ qh.abs() + Lq * E * AK), flat(AK), Lq, unit),
            "gv": Out(flat(Pp.transpose(-1, -2) @ gh), flat(dPp.transpose(-1, -2) @ gh.abs() + Lq * E * AV), flat(AV), Lq, unit)}


def mha_scale(dh):
    return float(np.float32(1.0 / math.sqrt(dh)))


# ---------------------------------------------------------------------------------------------------------------------------
# case lists (the GPU module's tables) and the inputs of each case: float64 tensors that hold fp32 (fp16) values

LN_CASES = [(1, 1), (1, 63), (3, 64), (5, 65), (15, 100), (16, 128), (17, 64), (33, 768), (4, 2048), (257, 65), (530, 64)]
MHA_CASES = [(1, 1, 1, 1, 1), (2, 3, 5, 2, 4), (3, 5, 3, 1, 7), (2, 64, 64, 2, 31), (2, 64, 64, 2, 32), (2, 33, 63, 1, 8),
             (2, 31, 65, 2, 8), (1, 90, 91, 1, 4), (1, 128, 64, 1, 2)]
MHA_DROP_CASES = [(2, 3, 5, 2, 4), (2, 64, 64, 2, 31), (2, 64, 64, 2, 32)]
MHA_DROP_P = [0.1, 0.5]
MHA_KLENS = ["Lk", "1", "0", "Lk-1", "Lk+3"]
# planted (b): (B, Lq, Lk, nh, dh), scale, key_len -- q = 0, P = 1 / klen, every klen and the scale a power of two
MHA_UNIFORM = [((2, 5, 8, 2, 4), 0.5, [8, 4]), ((2, 7, 16, 2, 16), 0.25, [2, 16]), ((2, 64, 64, 2, 32), 0.25, [64, 32]),
               ((2, 64, 64, 2, 31), 0.125, None)]
MHA_ONE_KEY = [(2, 3, 5, 2, 4), (2, 64, 64, 2, 31), (2, 64, 64, 2, 32), (1, 90, 91, 1, 4)]                  # planted (a)
SM_ROWS = [1, 3, 4, 5, 61]
SM_COLS = [(1, 1), (63, 64), (64, 64), (65, 128), (100, 128)]
MSE_CASES = [(1, 1), (3, 7), (4, 32), (43, 3), (37, 30)]
MSE_FORMS = ["plain", "loss", "pred", "both"]
HEAD_CASES = [(1, 1, 1, 1), (2, 5, 7, 2), (9, 7, 3, 2), (8, 8, 5, 3), (13, 5, 4, 1), (3, 30, 64, 2)]
NL_CASES = [(1, 1, 1, 1), (2, 3, 5, 7), (5, 8, 1, 7), (20, 3, 18, 30), (96, 4, 64, 64)]
NL_REALISTIC = [(2, 3, 5, 7), (20, 3, 18, 30)]
NL_LAYOUTS = ["bcs", "bsc", "bcs_padded"]
CONV_CASES = [(1, 1, 1, 1), (2, 3, 5, 1), (2, 3, 5, 2), (2, 3, 5, 3), (2, 3, 5, 4), (7, 3, 9, 2), (4, 2, 16, 4), (5, 3, 13, 3)]
POLY_CASES = [(1, 1, 1), (3, 5, 7), (5, 51, 2), (4, 64, 3), (257, 1, 2), (2, 300, 3)]
MM_CASES = [(1, 1, 1), (5, 17, 3), (4, 8, 8), (257, 1, 1)]
MM_LENS = ["-1", "0", "1", "P", "P+3"]
COLSUM_CASES = [(1, 1), (127, 63), (129, 65), (2049, 64)]
REGIMES = ["integer", "realistic"]


def len_value(name, P):
    return {"-1": -1, "0": 0, "1": 1, "P": P, "P+3": P + 3, "Lk": P, "Lk-1": P - 1, "Lk+3": P + 3}[name]


def rotated(names, B, shift, P):
    """slot b of call `shift` takes names[(b + shift) % 5]: over range(0, 5, B) every slot pattern appears"""
    return [len_value(names[(b + shift) % len(names)], P) for b in range(B)]


def make_ln(M, D):
    """N(0, 1) rows with the planted ones: row 0 constant 3 (its mean is exact: xhat == 0), row 1 1000 + N(0, 1), row 2 one spike"""
    g_ = gen(1000 + M * 2053 + D)
    x = data((M, D), "realistic", g_)
    x[0] = 3.0
    if M > 1:
        x[1] = (x[1] + 1000.0).float().double()
    if M > 2:
        x[2, D // 2] = 1.0e4
    gamma = (0.75 + ((torch.arange(D, dtype=F64) * 37) % 8209) / 8209).float().double()
    return dict(x=x, gamma=gamma, gy=data((M, D), "realistic", g_), gg0=data((D,), "realistic", g_), gb0=data((D,), "realistic", g_))


def make_mha(case, regime, klen=None):
    """realistic: q, k ~ N(0, 1), rows of k, v behind klen times 8 (a leak shows); integer: small integers"""
    B, Lq, Lk, nh, dh = case
    g_ = gen(2000 + sum(c * 31 ** i for i, c in enumerate(case)))
    r = 3 if regime == "integer" else 8
    q, go = data((B, Lq, nh, dh), regime, g_, r=r), data((B, Lq, nh, dh), regime, g_, r=r)
    k, v = data((B, Lk, nh, dh), regime, g_, r=r), data((B, Lk, nh, dh), regime, g_, r=r)
    if klen is not None and regime == "realistic":
        for b, n in enumerate(klen):
            k[b, max(n, 0):] *= 8
            v[b, max(n, 0):] *= 8
    return dict(q=q, k=k, v=v, go=go)


def make_sm(rows, nv, regime):
    g_ = gen(3000 + rows * 131 + nv)
    if regime == "integer":
        return dict(P=torch.full((rows, nv), 2.0 ** -7, dtype=F64), dP=ints((rows, nv), g_), scale=0.25, unit=0.25 * 2.0 ** -14)
    P = torch.softmax(torch.randn(rows, nv, generator=g_).double() * 2, 1).to(F16).double()
    return dict(P=P, dP=data((rows, nv), "realistic", g_), scale=mha_scale(96), unit=1.0)


def make_mse(B, To, regime):
    g_ = gen(4000 + B * 67 + To)
    if regime == "integer":   # mn = 0, r a power of two per coordinate, pred / gt multiples of 2^-10, seeds powers of two / multiples of 2^-4
        q = lambda: torch.randint(0, 1025, (B, 2, To), generator=g_).double() / 1024
        ns = torch.tensor([[0.0, 4.0, 0.0, 2.0]], dtype=F64).repeat(B, 1)
        return dict(pred=q(), gt=q(), ns=ns, g_loss=0.5, g_pred=ints((B, 2, To), g_) / 16, unit=2.0 ** -10 * 4 * 2 / (B * To) / 2)
    u = lambda *s: torch.rand(*s, generator=g_).float().double()
    mn = u(B, 2) * 3000 + 500
    ns = torch.stack([mn[:, 0], mn[:, 0] + 50 + u(B) * 400, mn[:, 1], mn[:, 1] + 1 + u(B) * 100], 1).float().double()
    return dict(pred=u(B, 2, To), gt=u(B, 2, To), ns=ns, g_loss=float(np.float32(0.37)), g_pred=data((B, 2, To), "realistic", g_), unit=1.0)


def make_head(case, regime):
    B, To, C, F = case
    g_ = gen(5000 + sum(c * 37 ** i for i, c in enumerate(case)))
    return dict(g=data((B, F, To), regime, g_), fused=data((B, To, C), regime, g_), w=data((F, C), regime, g_, C ** -0.5))


def make_nl(case, regime):
    B, C, T, S = case
    g_ = gen(6000 + sum(c * 41 ** i for i, c in enumerate(case)))
    return dict(inp=data((B, T, C), regime, g_), W=data((C, S, T), regime, g_, T ** -0.5), g=data((B, C, S), regime, g_))


def make_conv(case, regime):
    B, C, T, F = case
    g_ = gen(7000 + sum(c * 43 ** i for i, c in enumerate(case)))
    return dict(gxp=data((B, T, C), regime, g_), x=data((B, F, T), regime, g_))


def make_poly(case, regime):
    """pixel coordinates up to 3839 in both regimes; integer g in [-3, 3] keeps 600 * 3839 * 3 below 2^24"""
    B, P, D = case
    g_ = gen(8000 + sum(c * 47 ** i for i, c in enumerate(case)))
    if regime == "integer":
        poly = torch.randint(0, 3840, (B, P, 2), generator=g_).double()
        poly[0, 0, 0] = 3839.0
        return dict(g=torch.randint(-2, 3, (B, P, D), generator=g_).double() + (torch.arange(P) % 2).double()[None, :, None], poly=poly)
    return dict(g=data((B, P, D), regime, g_), poly=(torch.rand(B, P, 2, generator=g_) * 3839).float().double())


def make_colsum(M, N, dt):
    g_ = gen(9000 + M * 71 + N)
    return dict(g=ints((M, N), g_), init=ints((N,), g_))            # small integers are exact in bf16 too (|v| <= 20 < 256)
