"""The fp32 backward kernels of the trajectory head and the small encoders (csrc/backward.hip) per element against float64, each
called on its own: tcavt_layernorm_bwd, tcavt_mha_bwd, tcavt_softmax_bwd_rows, tcavt_mse_grad(_seeded), tcavt_out_head_bwd,
tcavt_nlinear_bwd, tcavt_conv1x1_bwd, tcavt_poly_embed_bwd, tcavt_masked_mean_bwd, tcavt_colsum (with reduce_partials_kernel).

Every case calls the C entry point (capi.lib().tcavt_*) and checks EVERY element against one float64 evaluation of the header's
formula in torch on the CPU (tests/head_backward_ref.py; test_head_backward_ref_cpu.py ties each closed form to float64 autograd and
shows that each checker fails on one moved element, two swapped rows, an unwritten tail element).  Nothing in a reference comes
from a project kernel: dropout masks are oracle/philox.py keep_mask(B nh Lq Lk, p, seed, site) at ((b nh + h) Lq + i) Lk + j,
1 / (1 - p) is the fp32 quotient of make_dropout.

Buffers: every output lies in a larger NaN-filled allocation with guard rows before and after (and a padded leading dimension with
sentinel columns where the entry takes one), every input in a buffer with NaN rows behind it: every in-range element must come back
finite and inside its bound, every guard element keep its bits, every input stay bit-unchanged, a second launch give the same
bits.  The workspaces of layernorm_bwd and colsum are exactly the documented size, NaN on the first launch, large finite garbage on
the second.

Two regimes:
- integer (out_head_bwd, nlinear_bwd, conv1x1_bwd, poly_embed_bwd, colsum; planted cases of mha_bwd, softmax_bwd_rows, mse_grad):
  small-integer operands (or multiples of a power of two), distinct per index; the sums of absolute values are asserted below
  2^24 units on the CPU, so fp32 is exact in any order and got must EQUAL the float64 value rounded to the output type.
- realistic: N(0, 1)-like data,  |got - ref| <= 1.01 * [fp32 terms] + ulp_out(ref), the fp32 terms n * 2^-24 * sum |terms| with the
  chain length n read from the kernel and written next to each reference in head_backward_ref.py; LayerNorm carries its
  cancellation terms.  Bounds come from float64 intermediates of the reference alone; no constant is tuned to a measurement.

| kernel | shapes | reaches |
|---|---|---|
| layernorm_bwd (M, D) | (1,1) (1,63) (3,64) (5,65) (15,100) (16,128) (17,64) (33,768) (4,2048) (257,65) (530,64) | D = 1 (variance 0); the lane stride at 63 / 64 / 65; 15 / 16 / 17 rows on the 16-row block edge; M % 4 != 0 under the wave stride; the D limit; nb = 17 and 34 partials: reducer waves with 2 and 3 rows, one short, the trailing ones empty.  ggamma / gbeta accumulate onto a non-zero start; rows: constant (xhat == 0 exactly), 1000 + N(0, 1), one spike of 1e4 |
| mha_bwd (B, Lq, Lk, nh, dh) | (1,1,1,1,1) (2,3,5,2,4) (3,5,3,1,7) (2,64,64,2,31) (2,64,64,2,32) (2,33,63,1,8) (2,31,65,2,8) (1,90,91,1,4) (1,128,64,1,2) | Lq != Lk both ways; dh = 31 the last staged and dh = 32 the first unstaged shape at 64 x 64; Lk = 63 / 65 around the lane stride; Lq > 64 under the wave stride; 128 x 64 exactly 64 KiB of P / dS.  Separate padded ldq / ldk / ldv / ldo / ldg; key_len NULL and ragged {Lk, 1, 0, Lk - 1, Lk + 3} in every batch slot: masked keys get exactly zero dK / dV, key_len 0 all-zero gradients |
| mha_bwd planted | (a) key_len = 1 at (2,3,5,2,4) (2,64,64,2,31) (2,64,64,2,32) (1,90,91,1,4), p = 0 and 0.5: P == 1, dQ = dK = 0, dV[0] = sum_i keep_i / (1 - p) dO[i] in integers.  (b) q = 0, klen and scale powers of two at (2,5,8,2,4) (2,7,16,2,16) (2,64,64,2,32) (2,64,64,2,31): P = 1 / klen, dQ and dV equal float64 bit for bit, dK = 0.  Both rest on __expf(0) == 1, which the device gives (the cases pass exactly) |
| mha_bwd dropout | p = 0.1, 0.5 at (2,3,5,2,4) (2,64,64,2,31) (2,64,64,2,32); the masks both keep and drop |
| softmax_bwd_rows (rows, n_valid, n_out) | rows 1, 3, 4, 5, 61 x (1,1) (63,64) (64,64) (65,128) (100,128) | 4 rows per block; the lane stride; n_out == n_valid; padding written as +0; padded ldp / ldd / lds, columns >= n_out keep the sentinel; planted P = 2^-7 with integer dP: bit-equal to bf16(float64) |
| mse_grad, mse_grad_seeded (B, To) | (1,1) (3,7) (4,32) (43,3) (37,30) | B 2 To = 256 exactly, and 258; all four instantiations; g_loss = 1 alone gives the bits of mse_grad; exact plant at (4,32) |
| out_head_bwd (B, To, C, F) | (1,1,1,1) (2,5,7,2) (9,7,3,2) (8,8,5,3) (13,5,4,1) (3,30,64,2) | B To = 63 / 64 / 65 in the wave loop of gw / gb; F = 1, 2, 3 |
| nlinear_bwd (B, C, T, S) | (1,1,1,1) (2,3,5,7) (5,8,1,7) (20,3,18,30) (96,4,64,64) | T = 1; S T and B (T - 1) > 256; exactly 64 KiB of LDS; g as (C S, S, 1), (S C, 1, C) and with a padded batch stride; gin given and NULL (its buffer untouched) |
| conv1x1_bwd (B, C, T, F) | (1,1,1,1) (2,3,5,1..4) (7,3,9,2) (4,2,16,4) (5,3,13,3) | B T = 63 / 64 / 65; every F |
| poly_embed_bwd (B, P, D) | (1,1,1) (3,5,7) (5,51,2) (4,64,3) (257,1,2) (2,300,3) | B P = 255 / 256 / 257 around the 256-thread tree; P > 256: the second round of the gpos loop; pixel coordinates up to 3839 |
| masked_mean_bwd (B, P, D) | (1,1,1) (5,17,3) (4,8,8) (257,1,1) | B P D = 255 / 256 / 257; len -1, 0, 1, P, P + 3 in every batch slot; bit-equal to one fp32 division |
| colsum (M, N), fp32 and bf16 | (1,1) (127,63) (129,65) (2049,64) | integer regime (test_backward_kernels_gpu.py has the realistic one); nb = 17 partials; padded ld; accumulate 0 / 1 |

Refusals pass only what the host rejects before any launch: non-zero status, tcavt_last_error names the entry, outputs keep their
bits.  Failing cases found by this module: none so far.

MEASURED on an MI355X: profiles/head_backward_bounds.txt has the worst fraction of the bound per kernel and output with the chain
length n; test_report_worst_ratio prints the session's (pytest -s).  Worst fraction of the whole bound (bar 1.0), realistic cases:
  tcavt_layernorm_bwd    gx 0.219  ggamma 0.082  gbeta 0.083        tcavt_out_head_bwd    gf 0.411  gw 0.101  gb 0.048
  tcavt_mha_bwd          staged gq 0.024 gk 0.026 gv 0.049; unstaged 0.025 0.013 0.016; dropout <= 0.064
  tcavt_softmax_bwd_rows dS 0.500 (the bf16 rounding)               tcavt_nlinear_bwd     gW 0.480  gbias 0.216  gin 0.169
  tcavt_mse_grad         0.877 plain, 0.876 g_loss, 0.874 both      tcavt_conv1x1_bwd     gw 0.182  gb 0.076
  tcavt_masked_mean_bwd  0.471 (and bit-equal)                      tcavt_poly_embed_bwd  gw 0.058  gb 0.038  gpos 0.248
Where a fraction is tiny (mha_bwd, the gb sums, ggamma / gbeta) the bound is a worst-case chain, not a rounding test: the integer
regime carries the index coverage there.
Mutants (one in-bounds line each, built off-tree; profiles/head_backward_bounds.txt): out_head_bwd_w_kernel summing i < B To - 1,
nlinear_bwd_kernel leaving gin[.., T - 2] unwritten, the dK / dV loop over j < klen - 1, reduce_partials_kernel with per = nb / 16:
each fails here; test_backward_kernels_gpu.py passes the second (an unwritten NaN drops out of its max()).
"""
import pytest
import torch

import head_backward_ref as R
from head_backward_ref import (COLSUM_CASES, CONV_CASES, HEAD_CASES, LN_CASES, MHA_CASES, MHA_DROP_CASES, MHA_DROP_P, MHA_KLENS,
                               MHA_ONE_KEY, MHA_UNIFORM, MM_CASES, MM_LENS, MSE_CASES, MSE_FORMS, NL_CASES, NL_LAYOUTS, NL_REALISTIC,
                               POLY_CASES, REGIMES, SM_COLS, SM_ROWS, mha_staged)
from test_attention_bwd_gpu import _first_bad, _same_bits          # noqa: F401  (the house helpers: imported, not copied)
from test_forward_row_kernels_gpu import _bits_equal, _guarded, _refused
from test_gemm_forms_gpu import Poisoned, _dt_code, _ulp           # noqa: F401
from test_head_forward_kernels_gpu import _dev, _ins, _p, _twice
from test_llm_backward_kernels_gpu import Guarded, _L, _st, _unchanged   # noqa: F401

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
SITE = 41
_WORST = {}   # (kernel, output) -> (worst fraction, chain length)


def _cdiv(a, b):
    return -(-a // b)


def _judge(got, out, regime, what, kernel, name):
    frac = R.check(got, out, regime, what)
    if regime == "realistic":
        print(f"frac {what} {name} (n = {out.n}): {frac:.3f}")
        w = _WORST.get((kernel, name), (-1.0, 0))
        _WORST[(kernel, name)] = (max(w[0], frac), max(w[1], out.n))


def _padded(rows, cols, dt, dev, pad=8):
    """an output region with a padded leading dimension: sentinel (NaN) columns behind every row, eight guard rows on each side"""
    return Guarded(rows, cols, dt, dev, ld=cols + pad, before=8, after=8)


def _workspace(n, dev, second):
    """exactly n floats between guards: NaN on the first launch, large finite garbage on the second"""
    ws = Guarded(1, n, F32, dev, before=4, after=4)
    if second:
        ws.region.copy_((torch.randn(1, n, generator=R.gen(n)) * 1e6).to(dev))
    return ws


def _counted(make):
    """make(second) -> outputs, as the make_outs of _twice: the first call gets second = False"""
    calls = []

    def f():
        calls.append(1)
        return make(len(calls) > 1)
    return f


def test_cases_cover_the_host_rules():
    """from the case lists alone (the launch arithmetic of the entry points mirrored): every boundary is reached on both sides"""
    # layernorm_bwd: one block per 16 rows, a wave per row (rows w, w + 4, ..), lanes stride 64 over D <= 2048; nb partial rows
    # reduced by 16 waves of ceil(nb / 16) rows each
    Ms, Ds = {M for M, _ in LN_CASES}, {D for _, D in LN_CASES}
    assert {1, 63, 64, 65, 2048} <= Ds and {15, 16, 17} <= Ms and any(M % 4 for M in Ms) and max(Ds) == 2048
    ranges = {}
    for M in Ms:
        nb = _cdiv(M, 16)
        per = _cdiv(nb, 16)
        ranges[nb] = [max(0, min(nb, w * per + per) - min(nb, w * per)) for w in range(16)]
    assert ranges[17] == [2] * 8 + [1] + [0] * 7 and ranges[34] == [3] * 11 + [1] + [0] * 4 and ranges[1] == [1] + [0] * 15
    # mha_bwd: P and dS in LDS (refused beyond 64 KiB), q / k / v / dO staged beside them when that fits too
    assert all(2 * Lq * Lk * 4 <= 65536 for _, Lq, Lk, _, _ in MHA_CASES)
    assert 2 * 64 * 64 * 4 + 2 * 128 * 32 * 4 == 65536 and mha_staged(64, 64, 31) and not mha_staged(64, 64, 32)
    kinds = {c: mha_staged(c[1], c[2], c[4]) for c in MHA_CASES}
    assert kinds[(1, 1, 1, 1, 1)] and kinds[(2, 33, 63, 1, 8)] and kinds[(2, 31, 65, 2, 8)] and not kinds[(1, 90, 91, 1, 4)]
    assert 2 * 128 * 64 * 4 == 65536 and not kinds[(1, 128, 64, 1, 2)]
    assert any(Lq < Lk for _, Lq, Lk, _, _ in MHA_CASES) and any(Lq > Lk for _, Lq, Lk, _, _ in MHA_CASES)
    assert {63, 65} <= {Lk for _, _, Lk, _, _ in MHA_CASES} and any(Lq > 64 for _, Lq, _, _, _ in MHA_CASES)
    for c in MHA_CASES:                # every key_len pattern reaches every batch slot of every shape
        assert {(b + s) % 5 for s in range(0, 5, c[0]) for b in range(c[0])} == set(range(5))
    assert {mha_staged(c[1], c[2], c[4]) for c in MHA_DROP_CASES} == {True, False} and set(MHA_DROP_CASES) <= set(MHA_CASES)
    assert {mha_staged(c[1], c[2], c[4]) for c in MHA_ONE_KEY} == {True, False}
    assert {mha_staged(c[1], c[2], c[4]) for c, _, _ in MHA_UNIFORM} == {True, False}
    for c, scale, kl in MHA_UNIFORM:   # powers of two
        assert all(n & (n - 1) == 0 and 0 < n <= c[2] for n in (kl or [c[2]])) and torch.frexp(torch.tensor(scale))[0].item() == 0.5
    # softmax_bwd_rows: 4 rows per block, lanes stride 64 over n_valid and n_out
    assert {r % 4 for r in SM_ROWS} == {0, 1, 3} and 1 in SM_ROWS and max(SM_ROWS) > 4
    assert {nv for nv, _ in SM_COLS} >= {1, 63, 64, 65} and any(nv == no for nv, no in SM_COLS) and any(no - nv > 0 for nv, no in SM_COLS)
    # mse_grad: one thread per element of [B, 2, To], 256-thread blocks
    n = [B * 2 * To for B, To in MSE_CASES]
    assert n[0] == 2 and 256 in n and 258 in n and max(n) > 2 * 256 and set(MSE_FORMS) == {"plain", "loss", "pred", "both"}
    # out_head_bwd: gf one thread per element; gw / gb one wave per output, lanes stride 64 over B To
    assert {63, 64, 65} <= {B * To for B, To, _, _ in HEAD_CASES} and {1, 2, 3} <= {F for _, _, _, F in HEAD_CASES}
    assert any(B * To * C > 256 for B, To, C, _ in HEAD_CASES)
    # nlinear_bwd: a block of 256 threads per channel, (B (T + S) + S T) * 4 bytes of LDS <= 64 KiB
    lds = [(B * (T + S) + S * T) * 4 for B, _, T, S in NL_CASES]
    assert max(lds) == 65536 and any(T == 1 for _, _, T, _ in NL_CASES)
    assert any(S * T > 256 for _, _, T, S in NL_CASES) and any(B * (T - 1) > 256 for B, _, T, _ in NL_CASES) and set(NL_REALISTIC) <= set(NL_CASES)
    # conv1x1_bwd: a wave per channel, lanes stride 64 over B T; F <= 4
    assert {63, 64, 65} <= {B * T for B, _, T, _ in CONV_CASES} and {F for _, _, _, F in CONV_CASES} == {1, 2, 3, 4}
    # poly_embed_bwd: a block of 256 threads per column d, threads stride 256 over B P (tree) and over P (gpos)
    assert {255, 256, 257} <= {B * P for B, P, _ in POLY_CASES} and any(P > 256 for _, P, _ in POLY_CASES)
    # masked_mean_bwd: one thread per element
    assert {255, 256, 257} <= {B * P * D for B, P, D in MM_CASES}
    for B, _, _ in MM_CASES:
        assert {(b + s) % 5 for s in range(0, 5, B) for b in range(B)} == set(range(5))
    assert [R.len_value(v, 8) for v in MM_LENS] == [-1, 0, 1, 8, 11]
    # colsum: 128 rows per block and 64 columns; nb partial rows
    assert {_cdiv(M, 128) for M, _ in COLSUM_CASES} == {1, 2, 17} and {63, 64, 65} <= {N for _, N in COLSUM_CASES}


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_colsum, tcavt_layernorm_bwd

@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,N", COLSUM_CASES)
@pytest.mark.gpu
def test_colsum(gpu, M, N, dt):
    dev = gpu["device"]
    d = R.make_colsum(M, N, dt)
    g = Poisoned(M, N, dt, dev, ld=N + 13, extra_rows=3, fill=d["g"])
    assert torch.equal(g.region.double().cpu(), d["g"])
    nb = _cdiv(M, 128)
    for acc in (0, 1):
        what = f"colsum {(M, N)} {dt} accumulate={acc}"
        out, ws = _twice(lambda out, ws: _L().tcavt_colsum(g.buf.data_ptr(), g.ld, _dt_code(dt), out.ptr, M, N, acc, ws.ptr, nb * N, _st()),
                         _counted(lambda second: (_guarded(1, N, F32, dev, fill=d["init"][None] if acc else None), _workspace(nb * N, dev, second))),
                         _ins(g=g), what)
        _judge(out.region, R.colsum_ref(d["g"], d["init"] if acc else None)["out"], "integer", what, "tcavt_colsum", "out")


@pytest.mark.parametrize("M,D", LN_CASES)
@pytest.mark.gpu
def test_layernorm_bwd(gpu, M, D):
    dev = gpu["device"]
    d = R.make_ln(M, D)
    x, gamma, gy = _dev(d["x"], dev), _dev(d["gamma"][None], dev), _dev(d["gy"], dev)
    n_ws = _cdiv(M, 16) * 2 * D
    what = f"layernorm_bwd {(M, D)}"
    gx, gg, gb, _ = _twice(lambda gx, gg, gb, ws: _L().tcavt_layernorm_bwd(x.buf.data_ptr(), gamma.buf.data_ptr(), gy.buf.data_ptr(), R.LN_EPS, gx.ptr,
                                                                          gg.ptr, gb.ptr, M, D, ws.ptr, n_ws, _st()),
                           _counted(lambda second: (_guarded(M, D, F32, dev), _guarded(1, D, F32, dev, fill=d["gg0"][None]),
                                                    _guarded(1, D, F32, dev, fill=d["gb0"][None]), _workspace(n_ws, dev, second))),
                           _ins(x=x, gamma=gamma, gy=gy), what)
    o = R.layernorm_bwd_ref(**d)
    for name, t in (("gx", gx), ("ggamma", gg), ("gbeta", gb)):
        _judge(t.region, o[name], "realistic", what, "tcavt_layernorm_bwd", name)
    # the constant row: xhat == 0 exactly, so its gx is rstd (gy gamma - mean(gy gamma)) and it adds exactly nothing to ggamma:
    # with M == 1 ggamma comes back as its start, bit for bit
    if M == 1:
        _bits_equal(gg.region, d["gg0"][None].float(), what + ": a constant row moved ggamma")


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_mha_bwd

def _mha_run(dev, case, d, kl, scale, p, regime, what, unit=1.0):
    """one checked call pair; kl None (key_len NULL) or the raw key_len values (clamped to Lk by the kernel and by the reference)"""
    from tcavt_amd import ops

    B, Lq, Lk, nh, dh = case
    Em = nh * dh
    ops.set_dropout_epoch(None)        # masks are a function of (seed, site, element) alone
    q = Poisoned(B * Lq, Em, F32, dev, ld=Em + 8, extra_rows=3, fill=d["q"].reshape(B * Lq, Em))
    k = Poisoned(B * Lk, Em, F32, dev, ld=Em + 4, extra_rows=3, fill=d["k"].reshape(B * Lk, Em))
    v = Poisoned(B * Lk, Em, F32, dev, ld=Em + 12, extra_rows=3, fill=d["v"].reshape(B * Lk, Em))
    go = Poisoned(B * Lq, Em, F32, dev, ld=Em + 16, extra_rows=3, fill=d["go"].reshape(B * Lq, Em))
    ins = _ins(q=q, k=k, v=v, dO=go)
    ln = None
    if kl is not None:
        ln = torch.tensor([-7] + list(kl) + [Lk], dtype=torch.int32, device=dev)      # (neighbours that a wrong index would read)
        ins.append(("key_len", ln, ln.clone()))
    gq, gk, gv = _twice(lambda gq, gk, gv: _L().tcavt_mha_bwd(q.buf.data_ptr(), q.ld, k.buf.data_ptr(), k.ld, v.buf.data_ptr(), v.ld,
                                                               go.buf.data_ptr(), go.ld, gq.ptr, gk.ptr, gv.ptr, gq.ld,
                                                               None if ln is None else ln[1:].data_ptr(), B, Lq, Lk, nh, dh, scale,
                                                               p, R.SEED, SITE, _st()),
                        lambda: (_padded(B * Lq, Em, F32, dev), _padded(B * Lk, Em, F32, dev), _padded(B * Lk, Em, F32, dev)), ins, what)
    keep = R.attn_keep(B, nh, Lq, Lk, p, SITE) if p else None
    if p:
        assert 0 < keep.sum().item() < keep.numel(), what + ": the mask must both keep and drop"
    klen = [Lk] * B if kl is None else [min(max(n, 0), Lk) for n in kl]
    o = R.mha_bwd_ref(d["q"], d["k"], d["v"], d["go"], klen, scale, keep, R.inv_keep(p), unit)
    kernel = "tcavt_mha_bwd " + ("staged" if mha_staged(Lq, Lk, dh) else "unstaged") + (" dropout" if p else "")
    for name, t in (("gq", gq), ("gk", gk), ("gv", gv)):
        _judge(t.region, o[name], regime, what, kernel, name)
    for b, n in enumerate(klen):       # masked keys: exactly zero dK / dV; no key: all-zero gradients
        for name, t in (("gk", gk), ("gv", gv)):
            assert bool((t.region.reshape(B, Lk, Em)[b, n:] == 0).all()), f"{what}: {name} of a masked key is not zero (sample {b})"
        if n == 0:
            assert bool((gq.region.reshape(B, Lq, Em)[b] == 0).all()), f"{what}: key_len 0 must give zero dQ (sample {b})"
    return o, (gq, gk, gv)


@pytest.mark.parametrize("case", MHA_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.gpu
def test_mha_bwd(gpu, case):
    dev = gpu["device"]
    B, Lq, Lk, nh, dh = case
    _mha_run(dev, case, R.make_mha(case, "realistic"), None, R.mha_scale(dh), 0.0, "realistic", f"mha_bwd {case} key_len=NULL")
    for shift in range(0, 5, B):
        kl = R.rotated(MHA_KLENS, B, shift, Lk)
        _mha_run(dev, case, R.make_mha(case, "realistic", kl), kl, R.mha_scale(dh), 0.0, "realistic", f"mha_bwd {case} key_len={kl}")


@pytest.mark.parametrize("p", MHA_DROP_P)
@pytest.mark.parametrize("case", MHA_DROP_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.gpu
def test_mha_bwd_dropout(gpu, case, p):
    dev = gpu["device"]
    B, Lq, Lk, nh, dh = case
    _mha_run(dev, case, R.make_mha(case, "realistic"), None, R.mha_scale(dh), p, "realistic", f"mha_bwd {case} p={p}")
    kl = R.rotated(MHA_KLENS, B, 3, Lk)
    _mha_run(dev, case, R.make_mha(case, "realistic", kl), kl, R.mha_scale(dh), p, "realistic", f"mha_bwd {case} p={p} key_len={kl}")


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("case", MHA_ONE_KEY, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.gpu
def test_mha_bwd_one_key_exact(gpu, case, p):
    """planted (a): key_len = 1, P == 1: dQ = dK = 0 and dV[0] = sum_i keep_i / (1 - p) dO[i], exact in integers (1 / (1 - 0.5) = 2)"""
    dev = gpu["device"]
    B, Lq, Lk, nh, dh = case
    d = R.make_mha(case, "integer")
    o, (gq, gk, gv) = _mha_run(dev, case, d, [1] * B, R.mha_scale(dh), p, "integer", f"mha_bwd one key {case} p={p}")
    assert bool((gq.region == 0).all()) and bool((gk.region == 0).all())
    keep = R.attn_keep(B, nh, Lq, Lk, p, SITE)[:, :, :, 0] * R.inv_keep(p) if p else torch.ones(B, nh, Lq, dtype=F64)
    want = torch.einsum("bhi,bihe->bhe", keep, d["go"]).reshape(B, nh * dh)
    assert torch.equal(gv.region.reshape(B, Lk, nh * dh)[:, 0].double().cpu(), want)


@pytest.mark.parametrize("case,scale,kl", MHA_UNIFORM, ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else None)
@pytest.mark.gpu
def test_mha_bwd_uniform_exact(gpu, case, scale, kl):
    """planted (b): q = 0, every score 0, P = 1 / klen with klen and the scale powers of two: every product and partial sum is a
    whole number of scale / Lk^2 below 2^24 of them (asserted), so dQ and dV equal float64 and dK = 0"""
    dev = gpu["device"]
    B, Lq, Lk, nh, dh = case
    d = R.make_mha(case, "integer")
    d["q"] = torch.zeros_like(d["q"])
    pre = torch.einsum("bihe,bjhe->bhij", d["go"].abs(), d["v"].abs()).max().item() * Lk * Lk
    assert pre < 2.0 ** 24
    o, (gq, gk, gv) = _mha_run(dev, case, d, kl, scale, 0.0, "integer", f"mha_bwd uniform {case} key_len={kl}", unit=scale / Lk ** 2)
    assert bool((gk.region == 0).all()) and bool((o["gq"].ref != 0).any())


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_softmax_bwd_rows, tcavt_mse_grad(_seeded)

@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("nv,no", SM_COLS)
@pytest.mark.parametrize("rows", SM_ROWS)
@pytest.mark.gpu
def test_softmax_bwd_rows(gpu, rows, nv, no, regime):
    dev = gpu["device"]
    d = R.make_sm(rows, nv, regime)
    P = Poisoned(rows, nv, F16, dev, ld=no + 24, extra_rows=3, fill=d["P"])
    assert torch.equal(P.region.double().cpu(), d["P"])
    dP = Poisoned(rows, nv, F32, dev, ld=no + 8, extra_rows=3, fill=d["dP"])
    what = f"softmax_bwd_rows {(rows, nv, no)} {regime}"
    (dS,) = _twice(lambda dS: _L().tcavt_softmax_bwd_rows(P.buf.data_ptr(), P.ld, dP.buf.data_ptr(), dP.ld, dS.ptr, dS.ld, d["scale"], rows, nv, no, _st()),
                   lambda: (_padded(rows, no, BF16, dev, pad=16),), _ins(P=P, dP=dP), what)
    _judge(dS.region, R.softmax_bwd_rows_ref(d["P"], d["dP"], d["scale"], no, d["unit"])["dS"], regime, what, "tcavt_softmax_bwd_rows", "dS")
    _bits_equal(dS.region[:, nv:], torch.zeros(rows, no - nv, dtype=BF16), what + ": the padding is not +0")


@pytest.mark.parametrize("form", MSE_FORMS)
@pytest.mark.parametrize("B,To", MSE_CASES)
@pytest.mark.gpu
def test_mse_grad(gpu, B, To, form):
    dev = gpu["device"]
    for regime in ["realistic"] + (["integer"] if (B, To) == (4, 32) else []):
        d = R.make_mse(B, To, regime)
        pred, gt, ns, gp = (_dev(d[k].reshape(B, -1), dev) for k in ("pred", "gt", "ns", "g_pred"))
        gl = torch.tensor([NAN, d["g_loss"], NAN], dtype=F32, device=dev)
        ins = _ins(pred=pred, gt=gt, norm_stat=ns, g_pred=gp) + [("g_loss", gl, gl.clone())]
        pp, pg, pn = pred.buf.data_ptr(), gt.buf.data_ptr(), ns.buf.data_ptr()
        launch = {"plain": lambda g: _L().tcavt_mse_grad(pp, pg, pn, g.ptr, B, To, _st()),
                  "loss": lambda g: _L().tcavt_mse_grad_seeded(pp, pg, pn, gl[1:].data_ptr(), None, g.ptr, B, To, _st()),
                  "pred": lambda g: _L().tcavt_mse_grad_seeded(None, None, None, None, gp.buf.data_ptr(), g.ptr, B, To, _st()),
                  "both": lambda g: _L().tcavt_mse_grad_seeded(pp, pg, pn, gl[1:].data_ptr(), gp.buf.data_ptr(), g.ptr, B, To, _st())}[form]
        what = f"mse_grad {form} {(B, To)} {regime}"
        (g,) = _twice(launch, lambda: (_guarded(B, 2 * To, F32, dev),), ins, what)
        o = R.mse_grad_ref(d["pred"], d["gt"], d["ns"], d["g_loss"] if form in ("loss", "both") else None,
                           d["g_pred"] if form in ("pred", "both") else None, d["unit"])["g"]
        _judge(g.region, o, regime, what, "tcavt_mse_grad " + form, "g")
        if form == "pred":
            _bits_equal(g.region, gp.region, what + ": not a copy of g_pred")
        if form == "loss":          # a unit seed gives the bits of tcavt_mse_grad
            one = torch.ones(1, dtype=F32, device=dev)
            (g1,) = _twice(lambda g: _L().tcavt_mse_grad_seeded(pp, pg, pn, one.data_ptr(), None, g.ptr, B, To, _st()),
                           lambda: (_guarded(B, 2 * To, F32, dev),), ins, what + " g_loss=1")
            (g0,) = _twice(lambda g: _L().tcavt_mse_grad(pp, pg, pn, g.ptr, B, To, _st()), lambda: (_guarded(B, 2 * To, F32, dev),), ins, what)
            _bits_equal(g1.region, g0.region, what + ": g_loss = 1 differs from mse_grad")


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_out_head_bwd, tcavt_nlinear_bwd, tcavt_conv1x1_bwd, tcavt_poly_embed_bwd, tcavt_masked_mean_bwd

@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.gpu
def test_out_head_bwd(gpu, case, regime):
    dev = gpu["device"]
    B, To, C, F = case
    d = R.make_head(case, regime)
    g, fused, w = _dev(d["g"].reshape(B * F, To), dev), _dev(d["fused"].reshape(B * To, C), dev), _dev(d["w"], dev)
    what = f"out_head_bwd {case} {regime}"
    gf, gw, gb = _twice(lambda gf, gw, gb: _L().tcavt_out_head_bwd(g.buf.data_ptr(), fused.buf.data_ptr(), w.buf.data_ptr(), gf.ptr, gw.ptr, gb.ptr,
                                                                   B, To, C, F, _st()),
                        lambda: (_guarded(B * To, C, F32, dev), _guarded(F, C, F32, dev), _guarded(1, F, F32, dev)), _ins(g=g, fused=fused, w=w), what)
    o = R.out_head_bwd_ref(**d)
    for name, t in (("gf", gf), ("gw", gw), ("gb", gb)):
        _judge(t.region, o[name], regime, what, "tcavt_out_head_bwd", name)


@pytest.mark.parametrize("with_gin", [1, 0])
@pytest.mark.parametrize("layout", NL_LAYOUTS)
@pytest.mark.parametrize("case", NL_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.gpu
def test_nlinear_bwd(gpu, case, layout, with_gin):
    dev = gpu["device"]
    B, C, T, S = case
    for regime in ["integer"] + (["realistic"] if case in NL_REALISTIC else []):
        d = R.make_nl(case, regime)
        inp, W = _dev(d["inp"].reshape(B * T, C), dev), _dev(d["W"].reshape(C * S, T), dev)
        if layout == "bsc":
            g, strides = _dev(d["g"].permute(0, 2, 1).reshape(B, S * C), dev), (S * C, 1, C)
        else:
            pad = 5 if layout == "bcs_padded" else 0
            g = Poisoned(B, C * S, F32, dev, ld=C * S + pad, extra_rows=3, fill=d["g"].reshape(B, C * S))
            strides = (C * S + pad, S, 1)
        what = f"nlinear_bwd {case} {layout} gin={with_gin} {regime}"
        # gin == NULL: the kernel gets no pointer to it; a guarded buffer stands by and must keep every bit
        gW, gbias, gin = _twice(lambda gW, gbias, gin: _L().tcavt_nlinear_bwd(inp.buf.data_ptr(), W.buf.data_ptr(), g.buf.data_ptr(), *strides, gW.ptr,
                                                                             gbias.ptr, gin.ptr if with_gin else None, B, C, T, S, _st()),
                                lambda: (_guarded(C * S, T, F32, dev), _guarded(C, S, F32, dev), _guarded(B * T, C, F32, dev)),
                                _ins(in_tok=inp, W=W, g=g), what)
        o = R.nlinear_bwd_ref(**d)
        _judge(gW.region, o["gW"], regime, what, "tcavt_nlinear_bwd", "gW")
        _judge(gbias.region, o["gbias"], regime, what, "tcavt_nlinear_bwd", "gbias")
        if with_gin:
            _judge(gin.region, o["gin"], regime, what, "tcavt_nlinear_bwd", "gin")
        else:
            assert _same_bits(gin.buf, gin.before), what + ": gin == NULL, yet its buffer changed"
        if T == 1:
            assert bool((gW.region == 0).all()), what + ": u == 0 identically at T = 1"


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.gpu
def test_conv1x1_bwd(gpu, case, regime):
    dev = gpu["device"]
    B, C, T, F = case
    d = R.make_conv(case, regime)
    gxp, x = _dev(d["gxp"].reshape(B * T, C), dev), _dev(d["x"].reshape(B * F, T), dev)
    what = f"conv1x1_bwd {case} {regime}"
    gw, gb = _twice(lambda gw, gb: _L().tcavt_conv1x1_bwd(gxp.buf.data_ptr(), x.buf.data_ptr(), gw.ptr, gb.ptr, B, C, T, F, _st()),
                    lambda: (_guarded(C, F, F32, dev), _guarded(1, C, F32, dev)), _ins(gxp_tok=gxp, x=x), what)
    o = R.conv1x1_bwd_ref(**d)
    _judge(gw.region, o["gw"], regime, what, "tcavt_conv1x1_bwd", "gw")
    _judge(gb.region, o["gb"], regime, what, "tcavt_conv1x1_bwd", "gb")


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", POLY_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.gpu
def test_poly_embed_bwd(gpu, case, regime):
    dev = gpu["device"]
    B, P, D = case
    d = R.make_poly(case, regime)
    g, poly = _dev(d["g"].reshape(B * P, D), dev), _dev(d["poly"].reshape(B * P, 2), dev)
    what = f"poly_embed_bwd {case} {regime}"
    gw, gb, gpos = _twice(lambda gw, gb, gpos: _L().tcavt_poly_embed_bwd(g.buf.data_ptr(), poly.buf.data_ptr(), gw.ptr, gb.ptr, gpos.ptr, B, P, D, _st()),
                          lambda: (_guarded(D, 2, F32, dev), _guarded(1, D, F32, dev), _guarded(P, D, F32, dev)), _ins(g=g, polygon=poly), what)
    o = R.poly_embed_bwd_ref(**d)
    for name, t in (("gw", gw), ("gb", gb), ("gpos", gpos)):
        _judge(t.region, o[name], regime, what, "tcavt_poly_embed_bwd", name)


@pytest.mark.parametrize("case", MM_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.gpu
def test_masked_mean_bwd(gpu, case):
    dev = gpu["device"]
    B, P, D = case
    gemb64 = R.data((B, D), "realistic", R.gen(700 + B * P * D))
    gemb = _dev(gemb64, dev)
    for shift in range(0, 5, B):
        lens = R.rotated(MM_LENS, B, shift, P)
        ln = torch.tensor([P] + lens + [P], dtype=torch.int32, device=dev)           # (neighbours that a wrong index would read)
        what = f"masked_mean_bwd {case} len={lens if B <= 5 else lens[:5]}"
        (genc,) = _twice(lambda genc: _L().tcavt_masked_mean_bwd(gemb.buf.data_ptr(), ln[1:].data_ptr(), genc.ptr, B, P, D, _st()),
                         lambda: (_guarded(B * P, D, F32, dev),), _ins(gemb=gemb) + [("len", ln, ln.clone())], what)
        o = R.masked_mean_bwd_ref(gemb64, lens, P)["genc"]
        _judge(genc.region, o, "realistic", what, "tcavt_masked_mean_bwd", "genc")
        _bits_equal(genc.region.view(B, P, D), o.ref.float(), what + ": not one fp32 division (or not +0)")


# ---------------------------------------------------------------------------------------------------------------------------
# refusals

@pytest.mark.gpu
def test_refusals(gpu):
    """only what the host rejects before any launch"""
    dev = gpu["device"]
    d = torch.zeros(4096, device=dev).data_ptr()
    o1, o2, o3 = (_guarded(8, 64, F32, dev) for _ in range(3))
    outs = [o1, o2, o3]
    L, st = _L(), _st()
    # layernorm_bwd: NULL, D beyond the LDS slices, a workspace one float short
    _refused(L.tcavt_layernorm_bwd(d, d, None, 1e-5, o1.ptr, o2.ptr, o3.ptr, 4, 64, d, 128, st), "layernorm_bwd", outs, "gy NULL")
    _refused(L.tcavt_layernorm_bwd(d, d, d, 1e-5, o1.ptr, o2.ptr, o3.ptr, 1, 2049, d, 2 * 2049, st), "layernorm_bwd", outs, "D = 2049")
    _refused(L.tcavt_layernorm_bwd(d, d, d, 1e-5, o1.ptr, o2.ptr, o3.ptr, 17, 16, d, 2 * 2 * 16 - 1, st), "layernorm_bwd", outs, "workspace short")
    _refused(L.tcavt_layernorm_bwd(d, d, d, 1e-5, o1.ptr, o2.ptr, o3.ptr, 17, 16, None, 64, st), "layernorm_bwd", outs, "workspace NULL")
    # colsum
    _refused(L.tcavt_colsum(d, 8, _dt_code(F32), o1.ptr, 129, 8, 0, d, 2 * 8 - 1, st), "colsum", outs, "workspace short")
    _refused(L.tcavt_colsum(None, 8, _dt_code(F32), o1.ptr, 4, 8, 0, d, 8, st), "colsum", outs, "g NULL")
    # mha_bwd: NULL, P / dS beyond 64 KiB, dropout_p outside [0, 1)
    mha = lambda Lq, Lk, p, gk=o2.ptr: L.tcavt_mha_bwd(d, 8, d, 8, d, 8, d, 8, o1.ptr, gk, o3.ptr, 8, None, 1, Lq, Lk, 1, 2, 0.5, p, 1, 2, st)
    assert 128 * 65 * 8 > 65536
    _refused(mha(128, 65, 0.0), "mha_bwd", outs, "Lq Lk 8 > 64 KiB")
    _refused(mha(2, 2, 1.0), "mha_bwd", outs, "dropout_p = 1")
    _refused(mha(2, 2, -0.1), "mha_bwd", outs, "dropout_p = -0.1")
    _refused(mha(2, 2, 0.0, None), "mha_bwd", outs, "gk NULL")
    # softmax_bwd_rows, mse_grad
    _refused(L.tcavt_softmax_bwd_rows(d, 8, None, 8, o1.ptr, 8, 1.0, 2, 4, 4, st), "softmax_bwd_rows", outs, "dP NULL")
    _refused(L.tcavt_mse_grad(d, d, None, o1.ptr, 2, 2, st), "mse_grad", outs, "norm_stat NULL")
    _refused(L.tcavt_mse_grad_seeded(d, d, d, None, None, o1.ptr, 2, 2, st), "mse_grad_seeded", outs, "both seeds NULL")
    _refused(L.tcavt_mse_grad_seeded(None, d, d, d, None, o1.ptr, 2, 2, st), "mse_grad_seeded", outs, "g_loss without pred")
    # out_head_bwd, nlinear_bwd (LDS), conv1x1_bwd (F), poly_embed_bwd, masked_mean_bwd
    _refused(L.tcavt_out_head_bwd(d, d, None, o1.ptr, o2.ptr, o3.ptr, 2, 2, 2, 2, st), "out_head_bwd", outs, "w NULL")
    assert (97 * 128 + 4096) * 4 > 65536
    _refused(L.tcavt_nlinear_bwd(d, d, d, 256, 1, 4, o1.ptr, o2.ptr, None, 97, 4, 64, 64, st), "nlinear_bwd", outs, "LDS over 64 KiB")
    _refused(L.tcavt_nlinear_bwd(d, None, d, 4, 2, 1, o1.ptr, o2.ptr, None, 2, 2, 2, 2, st), "nlinear_bwd", outs, "W NULL")
    _refused(L.tcavt_conv1x1_bwd(d, d, o1.ptr, o2.ptr, 2, 2, 2, 5, st), "conv1x1_bwd", outs, "F = 5")
    _refused(L.tcavt_conv1x1_bwd(d, None, o1.ptr, o2.ptr, 2, 2, 2, 2, st), "conv1x1_bwd", outs, "x NULL")
    _refused(L.tcavt_poly_embed_bwd(d, None, o1.ptr, o2.ptr, o3.ptr, 2, 2, 2, st), "poly_embed_bwd", outs, "polygon NULL")
    _refused(L.tcavt_masked_mean_bwd(d, None, o1.ptr, 2, 2, 2, st), "masked_mean_bwd", outs, "len NULL")


@pytest.mark.gpu
def test_report_worst_ratio(gpu):
    """(runs last in file order) prints the worst fraction of the bound measured in this session per kernel and output"""
    for (k, name), (frac, n) in sorted(_WORST.items()):
        print(f"{k:34s} {name:7s} n = {n:3d}   worst frac {frac:7.4f}")
