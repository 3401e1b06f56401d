"""The forward kernels of the trajectory head (csrc/small.hip) against float64, each called on its own: tcavt_poly_embed,
tcavt_masked_mean, tcavt_ltsf_front, tcavt_ltsf_decode, tcavt_transpose_ct, tcavt_out_head.

Every case calls the C entry point (capi.lib().tcavt_*) and checks every element against ONE float64 evaluation of the header's
formula in torch on the CPU, from the same fp32 input values; nothing in a reference comes from a project kernel.  Every output lies
in a larger NaN-filled allocation with guard rows before and after, every input in a buffer with NaN rows behind it: every in-range
element must come back finite and inside its bound, every guard element keep its bits, every input stay bit-unchanged, a second
launch give the same bits.

Two regimes:
- integer (tcavt_poly_embed, tcavt_ltsf_front, tcavt_ltsf_decode, tcavt_out_head): small-integer operands, every partial sum an
  integer below 2^24 (asserted on the sums of absolute values), so the fp32 result is exact in any order and must equal the float64
  value: any wrong index changes it.
- realistic: N(0, 1)-like data, per-element bound derived next to each reference,
      |got - ref| <= 1.01 * [fp32 terms] + ulp_fp32(ref)
  with the chain length read from the kernel: the serial fmaf count plus the additions behind it (-ffp-contract=off: what is
  written as fmaf rounds once, everything else once per operation).
Exact functions are asserted by bits: xp_tok of tcavt_ltsf_front (the same two fmas and one addition, evaluated on the CPU),
tcavt_transpose_ct (a copy; the 16-bit output is the value rounded once), tcavt_masked_mean with len <= 0 (zeros).

| kernel | shapes | why |
|---|---|---|
| tcavt_poly_embed (B, P, D) | (1,1,1) (3,5,7) (2,64,64) (5,64,64) | one thread; one partial block; 32 and 80 whole blocks |
| tcavt_masked_mean (B, P, D) | the same | B * D = 320: a partial last block; len 0, 1, P, P + 3 (clamped to P), -1 (zeros) in every batch slot |
| tcavt_ltsf_front (B, C, T) | (1,1,1) (2,3,5) (3,64,17) (2,64,18) (2,64,19) | C * T below, and several times, the 256 threads of a sample's block; xp_tok NULL and given |
| tcavt_ltsf_decode (B, C, T, To) | (1,1,1,1) (2,3,5,7) (2,64,17,30) (3,64,18,30) (2,64,19,30) | T % 6 = 1, 5, 5, 0, 1: the unrolled loop never runs / runs with a tail of 5 / without a tail / with a tail of 1; 7.5 blocks per sample |
| tcavt_transpose_ct (B, C, To) | (1,1,1) (2,3,5) (3,64,30) | fp32, fp16, bf16 outputs, each alone and both |
| tcavt_out_head (B, To, C, F, T) | (1,1,1,1,1) (2,5,7,2,3) (3,30,64,2,18) | add_last 0 (x filled with NaN: the output stays finite) and 1 |

Refusals pass only arguments that the host code rejects before any launch: non-zero status, tcavt_last_error names the entry,
the outputs keep their bits (tcavt_ltsf_decode at T * C * 4 > 48 KiB, tcavt_ltsf_front at 8 T > 64 KiB, NULL pointers, a bad type).

MEASURED on an MI355X: the worst fraction of the whole bound per kernel stands beside the constants below;
profiles/forward_kernels_bounds.txt has every line, test_report_worst_ratio prints the session's (pytest -s).
"""
import pytest
import torch

from test_attention_bwd_gpu import _first_bad, _name, _same_bits
from test_forward_row_kernels_gpu import _bits_equal, _guarded, _refused
from test_gemm_forms_gpu import Poisoned, _dt_code, _round, _ulp
from test_llm_backward_kernels_gpu import _gen, _L, _ok, _st, _unchanged

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
_E = 2.0 ** -24   # unit roundoff of fp32
# MEASURED on an MI355X: worst fraction of the whole bound (bar 1.0) over the realistic cases (the integer regime is exact)
#   tcavt_ltsf_decode    0.161
#   tcavt_ltsf_front     0.126
#   tcavt_masked_mean    0.226
#   tcavt_out_head       0.220
#   tcavt_poly_embed     0.488
# Mutants (profiles/forward_kernels_bounds.txt): ltsf_decode without its tail loop (the earlier tests pass it), ltsf_front with
# last from T - 2, masked_mean dividing by P, out_head ignoring add_last: each fails here.
_WORST = {}

POLY_CASES = [(1, 1, 1), (3, 5, 7), (2, 64, 64), (5, 64, 64)]
LENS = ["0", "1", "P", "P+3", "-1"]
FRONT_CASES = [(1, 1, 1), (2, 3, 5), (3, 64, 17), (2, 64, 18), (2, 64, 19)]
DECODE_CASES = [(1, 1, 1, 1), (2, 3, 5, 7), (2, 64, 17, 30), (3, 64, 18, 30), (2, 64, 19, 30)]
TRANSPOSE_CASES = [(1, 1, 1), (2, 3, 5), (3, 64, 30)]
TRANSPOSE_OUTS = [(1, None), (0, F16), (0, BF16), (1, F16), (1, BF16)]      # (fp32 output, 16-bit output)
HEAD_CASES = [(1, 1, 1, 1, 1), (2, 5, 7, 2, 3), (3, 30, 64, 2, 18)]
REGIMES = ["integer", "realistic"]


def _len_value(name, P):
    return {"0": 0, "1": 1, "P": P, "P+3": P + 3, "-1": -1}[name]


def test_cases_cover_the_host_rules():
    """from the case lists alone (the launch arithmetic of the entry points mirrored): every path and edge is reached"""
    # poly_embed: one thread per element, 256-thread blocks
    n = [B * P * D for B, P, D in POLY_CASES]
    assert n[0] == 1 and 1 < n[1] < 256 and n[2] == 32 * 256 and n[3] == 80 * 256
    # masked_mean: one thread per (b, d); n = min(len, P) terms, zeros for n <= 0
    bd = [B * D for B, _, D in POLY_CASES]
    assert bd[0] == 1 and any(256 < v and v % 256 for v in bd)
    assert [_len_value(v, 64) for v in LENS] == [0, 1, 64, 67, -1]
    for B, _, _ in POLY_CASES:          # every length reaches every shape (over the calls of the test)
        assert {(b + s) % 5 for s in range(0, 5, B) for b in range(B)} == set(range(5))
    # ltsf_front: one block of 256 threads per sample, a thread per (c, s) in rounds of 256
    ct = [C * T for _, C, T in FRONT_CASES]
    assert ct[0] == 1 and ct[1] < 256 and all(v > 256 and v % 256 for v in ct[2:]) and {T for _, _, T in FRONT_CASES} >= {1, 17, 18, 19}
    # ltsf_decode: blocks of 256 outputs per sample; the weights in steps of six, then a tail loop
    assert [(T // 6, T % 6) for _, _, T, _ in DECODE_CASES] == [(0, 1), (0, 5), (2, 5), (3, 0), (3, 1)]
    assert any(C * To > 256 and (C * To) % 256 for _, C, _, To in DECODE_CASES) and all(T * C * 4 <= 48 * 1024 for _, C, T, _ in DECODE_CASES)
    # transpose_ct, out_head: one thread per output element
    assert [B * C * To for B, C, To in TRANSPOSE_CASES] == [1, 30, 22 * 256 + 128]
    assert {(f, h) for f, h in TRANSPOSE_OUTS} == {(1, None), (0, F16), (0, BF16), (1, F16), (1, BF16)}
    assert [B * F * To for B, To, _, F, _ in HEAD_CASES] == [1, 20, 180] and (3, 30, 64, 2, 18) in HEAD_CASES


def _data(shape, regime, g_, scale=1.0, r=3):
    """float64 on the CPU: integers in [-r, r] (integer regime) or N(0, scale^2)"""
    if regime == "integer":
        return torch.randint(-r, r + 1, shape, generator=g_).double()
    return torch.randn(shape, generator=g_).double() * scale


def _dev(t, dev):
    """t [rows, ...] as fp32 on the device with three NaN rows behind it; .region is the data (flattened to two dimensions)"""
    t2 = t.reshape(t.shape[0], -1)
    return Poisoned(t2.shape[0], t2.shape[1], F32, dev, ld=t2.shape[1], extra_rows=3, fill=t2)


def _ins(**kw):
    return [(k, v.buf, v.before) for k, v in kw.items()]


def _judge(got, ref, f32, absum, regime, what, kernel):
    """integer regime: exact (every partial sum below 2^24); realistic: |got - ref| <= 1.01 * f32 + ulp_fp32(ref)"""
    g = got.double().cpu().reshape(ref.shape)
    assert torch.isfinite(g).all(), f"{what}: {int((~torch.isfinite(g)).sum())} non-finite (unwritten?) elements in range"
    if regime == "integer":
        assert absum.max().item() < 2.0 ** 24
        bad = g != ref
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ; first {_first_bad(bad)}: got {g[_first_bad(bad)].item()!r} ref {ref[_first_bad(bad)].item()!r}"
        return
    bound = 1.01 * f32 + _ulp(ref, F32)
    d = (g - ref).abs()
    frac = (d / bound.clamp_min(1e-300)).max().item()
    _WORST[kernel] = max(_WORST.get(kernel, -1.0), frac)
    print(f"frac {what}: {frac:.3f}")
    bad = d > bound
    if bool(bad.any()):
        i = _first_bad(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of bound (worst fraction {frac:.3f}); first {i}: "
                             f"got {g[i].item()!r} ref {ref[i].item()!r} allowed {bound[i].item():.3e}")


def _twice(launch, make_outs, ins, what):
    """launch into fresh guarded outputs twice: guards, inputs, reproducibility; returns the first outputs"""
    runs = []
    for tag in ("", " again"):
        outs = make_outs()
        _ok(launch(*outs), what + tag)
        for o in outs:
            if o is not None:
                o.check(what + tag)
        _unchanged(ins, what + tag)
        runs.append(outs)
    for a, b in zip(*runs):
        assert a is None or _same_bits(a.region, b.region), what + ": not reproducible"
    return runs[0]


def _p(o):
    return o.ptr if o is not None else None


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_poly_embed, tcavt_masked_mean

@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("B,P,D", POLY_CASES)
def test_poly_embed(gpu, B, P, D, regime):
    """x[b][p][d] = fmaf(w[d][1], py, fmaf(w[d][0], px, 0)) + b_in[d] + pos[p][d]: four roundings, each of a partial sum bounded by
    U = |w0 px| + |w1 py| + |b_in| + |pos|: 4 E U"""
    dev = gpu["device"]
    g_ = _gen(100 + B * P * D)
    poly, w, bi, pos = (_dev(_data(s, regime, g_, sc), dev) for s, sc in (((B * P, 2), 300.0), ((D, 2), 0.05), ((1, D), 1.0), ((P, D), 1.0)))
    what = f"poly_embed {regime} {(B, P, D)}"
    (x,) = _twice(lambda x: _L().tcavt_poly_embed(poly.buf.data_ptr(), w.buf.data_ptr(), bi.buf.data_ptr(), pos.buf.data_ptr(), x.ptr, B, P, D, _st()),
                  lambda: (_guarded(B * P, D, F32, dev),), _ins(polygon=poly, w_in=w, b_in=bi, pos=pos), what)
    p64, w64, b64, s64 = (t.region.double().cpu() for t in (poly, w, bi, pos))
    a = p64[:, None, 0] * w64[None, :, 0]
    c = p64[:, None, 1] * w64[None, :, 1]
    posb = s64.repeat(B, 1)
    ref = a + c + b64 + posb
    U = a.abs() + c.abs() + b64.abs() + posb.abs()
    _judge(x.region, ref, 4 * _E * U, U, regime, what, "tcavt_poly_embed")


@pytest.mark.parametrize("B,P,D", POLY_CASES)
def test_masked_mean(gpu, B, P, D):
    """emb[b][d] = mean over p < min(len[b], P) of enc[b][p][d], exact zeros for len <= 0: n - 1 serial additions and the divide on
    mean|enc|: n E mean|enc|"""
    dev = gpu["device"]
    g_ = _gen(200 + B * P * D)
    enc = _dev(_data((B * P, D), "realistic", g_) + 0.5, dev)
    e64 = enc.region.double().cpu().view(B, P, D)
    for shift in range(0, 5, B):
        lens = [_len_value(LENS[(b + shift) % 5], P) for b in range(B)]
        ln = torch.tensor([-7] + lens + [P], dtype=torch.int32, device=dev)       # (neighbours that a wrong index would read)
        ln0 = ln.clone()
        what = f"masked_mean {(B, P, D)} len={lens}"
        (emb,) = _twice(lambda emb: _L().tcavt_masked_mean(enc.buf.data_ptr(), ln[1:].data_ptr(), emb.ptr, B, P, D, _st()),
                        lambda: (_guarded(B, D, F32, dev),), _ins(enc=enc) + [("len", ln, ln0)], what)
        ref, f32 = torch.zeros(B, D, dtype=F64), torch.zeros(B, D, dtype=F64)
        for b, n in enumerate(lens):
            n = min(n, P)
            if n > 0:
                ref[b] = e64[b, :n].mean(0)
                f32[b] = n * _E * e64[b, :n].abs().mean(0)
            else:
                assert bool((emb.region[b] == 0).all()) and not bool(torch.signbit(emb.region[b]).any()), what + f": sample {b} is not zeros"
        _judge(emb.region, ref, f32, f32, "realistic", what, "tcavt_masked_mean")


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_ltsf_front, tcavt_ltsf_decode

def _fma32(a, b, c):
    """fmaf(a, b, c) of fp32 values held in float64 tensors, as float32: a * b is exact in float64 (48 bits); the sum is rounded to
    odd there (two-sum residual), so that the second rounding to fp32 is the single rounding of the exact value"""
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(torch.int64) & 1) == 0
    toward = torch.where(err > 0, torch.full_like(s, float("inf")), torch.full_like(s, float("-inf")))
    s = torch.where((err != 0) & even, torch.nextafter(s, toward), s)
    return s.float()


def test_fma32_helper():
    one, u = torch.tensor([1.0], dtype=F64), 2.0 ** -24
    # 1 + 2^-24 is a tie (-> 1); a product that lies 2^-60 above / below it must round up / stay
    a, b = torch.tensor([2.0 ** -30], dtype=F64), torch.tensor([2.0 ** -30], dtype=F64)
    assert _fma32(a, b, one + u).item() == 1 + 2.0 ** -23 and _fma32(-a, b, one + u).item() == 1.0
    assert _fma32(a, 0 * b, one + u).item() == 1.0 and _fma32(torch.tensor([3.0], dtype=F64), torch.tensor([5.0], dtype=F64), one).item() == 16.0


def _xp_cpu(x64, cw64, cb64, B, C, T):
    """xp[b][c][t] = fmaf(w1, x[b][1][t], fmaf(w0, x[b][0][t], 0)) + cb[c] in fp32 arithmetic on the CPU"""
    x0, x1 = x64[:, None, 0, :].expand(B, C, T), x64[:, None, 1, :].expand(B, C, T)
    w0, w1 = cw64[None, :, 0, None].expand(B, C, T), cw64[None, :, 1, None].expand(B, C, T)
    t = _fma32(w0.contiguous(), x0.contiguous(), torch.zeros(B, C, T, dtype=F64))
    return _fma32(w1.contiguous(), x1.contiguous(), t.double()) + cb64.float()[None, :, None]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("B,C,T", FRONT_CASES)
def test_ltsf_front(gpu, B, C, T, regime):
    """xp = w0 x0 + w1 x1 + cb: three roundings of partial sums below U = |w0 x0| + |w1 x1| + |cb|: dxp = 3 E U (dlast at t = T - 1).
    diff = xp - last: ddiff = dxp + dlast + E |diff|.  acc = sum_t ew diff, T chained fmaf: sum |ew| ddiff + T E S, S = sum |ew| |diff|.
    acc + eb + last + pos: three additions, 3 E (S + |eb| + |last| + |pos|), and dlast."""
    dev = gpu["device"]
    g_ = _gen(300 + B * C * T)
    x, cw, cb = _dev(_data((B, 2, T), regime, g_), dev), _dev(_data((C, 2), regime, g_), dev), _dev(_data((1, C), regime, g_), dev)
    ew = _dev(_data((C, T, T), regime, g_, T ** -0.5), dev)
    eb, pos = _dev(_data((C, T), regime, g_), dev), _dev(_data((C, T), regime, g_), dev)
    ins = _ins(x=x, conv_w=cw, conv_b=cb, enc_w=ew, enc_b=eb, pos=pos)
    x64, cw64, cb64 = x.region.double().cpu().view(B, 2, T), cw.region.double().cpu(), cb.region.double().cpu().view(C)
    ew64, eb64, pos64 = ew.region.double().cpu().view(C, T, T), eb.region.double().cpu(), pos.region.double().cpu()
    a, c = cw64[None, :, 0, None] * x64[:, None, 0, :], cw64[None, :, 1, None] * x64[:, None, 1, :]          # [B, C, T]
    xp = a + c + cb64[None, :, None]
    U = a.abs() + c.abs() + cb64.abs()[None, :, None]
    last, dxp = xp[:, :, -1:], 3 * _E * U
    dlast = dxp[:, :, -1:]
    diff = xp - last
    ddiff = dxp + dlast + _E * diff.abs()
    acc = torch.einsum("cst,bct->bcs", ew64, diff)
    S = torch.einsum("cst,bct->bcs", ew64.abs(), diff.abs())
    ref = acc + eb64[None] + last + pos64[None]
    f32 = torch.einsum("cst,bct->bcs", ew64.abs(), ddiff) + T * _E * S + 3 * _E * (S + eb64.abs()[None] + last.abs() + pos64.abs()[None]) + dlast
    absum = S + eb64.abs()[None] + last.abs() + pos64.abs()[None] + U.max()
    for keep_xp in (False, True):
        what = f"ltsf_front {regime} {(B, C, T)} xp_tok={keep_xp}"
        tok, xpt = _twice(lambda tok, xpt: _L().tcavt_ltsf_front(x.buf.data_ptr(), cw.buf.data_ptr(), cb.buf.data_ptr(), ew.buf.data_ptr(),
                                                               eb.buf.data_ptr(), pos.buf.data_ptr(), tok.ptr, _p(xpt), B, C, T, _st()),
                          lambda: (_guarded(B * T, C, F32, dev), _guarded(B * T, C, F32, dev) if keep_xp else None), ins, what)
        _judge(tok.region.view(B, T, C).permute(0, 2, 1), ref, f32, absum, regime, what, "tcavt_ltsf_front")
        if keep_xp:
            _bits_equal(xpt.region.view(B, T, C).permute(0, 2, 1), _xp_cpu(x64, cw64, cb64, B, C, T), what + ": xp_tok is not the two fmas and the addition")


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("B,C,T,To", DECODE_CASES)
def test_ltsf_decode(gpu, B, C, T, To, regime):
    """diff = e - last rounds once (E |diff|); acc = sum_t dw diff, T chained fmaf: sum |dw| E |diff| + T E S, S = sum |dw| |diff|;
    acc + db + last + lane: three additions, 3 E (S + |db| + |last| + |lane|)"""
    dev = gpu["device"]
    g_ = _gen(400 + B * C * T * To)
    e, dw = _dev(_data((B, T, C), regime, g_), dev), _dev(_data((C, To, T), regime, g_, T ** -0.5), dev)
    db, lane = _dev(_data((C, To), regime, g_), dev), _dev(_data((B, C * To), regime, g_), dev)
    what = f"ltsf_decode {regime} {(B, C, T, To)}"
    (dec,) = _twice(lambda dec: _L().tcavt_ltsf_decode(e.buf.data_ptr(), dw.buf.data_ptr(), db.buf.data_ptr(), lane.buf.data_ptr(), dec.ptr,
                                                      B, C, T, To, _st()),
                    lambda: (_guarded(B, C * To, F32, dev),), _ins(e_tok=e, dec_w=dw, dec_b=db, lane_adj=lane), what)
    e64 = e.region.double().cpu().view(B, T, C).permute(0, 2, 1)                                             # [B, C, T]
    dw64, db64, lane64 = dw.region.double().cpu().view(C, To, T), db.region.double().cpu(), lane.region.double().cpu().view(B, C, To)
    last = e64[:, :, -1:]
    diff = e64 - last
    acc = torch.einsum("cst,bct->bcs", dw64, diff)
    S = torch.einsum("cst,bct->bcs", dw64.abs(), diff.abs())
    ref = acc + db64[None] + last + lane64
    rest = S + db64.abs()[None] + last.abs() + lane64.abs()
    f32 = _E * S + T * _E * S + 3 * _E * rest
    _judge(dec.region.view(B, C, To), ref, f32, rest + e64.abs().max() * 2, regime, what, "tcavt_ltsf_decode")


def test_ltsf_refusals(gpu):
    """tcavt_ltsf_decode stages e[b] ([T][C] fp32) in LDS and refuses T * C * 4 > 48 KiB; tcavt_ltsf_front stages x[b] ([2][T]) and
    refuses 8 T > 64 KiB -- both before the launch"""
    dev = gpu["device"]
    d = torch.zeros(64, device=dev).data_ptr()
    out, out2 = _guarded(4, 64, F32, dev), _guarded(4, 64, F32, dev)
    L = _L()
    _refused(L.tcavt_ltsf_decode(d, d, d, d, out.ptr, 1, 64, 193, 1, _st()), "ltsf_decode", [out], "T * C * 4 = 49408")
    _refused(L.tcavt_ltsf_decode(d, d, d, None, out.ptr, 1, 4, 4, 4, _st()), "ltsf_decode", [out], "lane_adj NULL")
    _refused(L.tcavt_ltsf_decode(d, d, d, d, out.ptr, 1, 4, 0, 4, _st()), "ltsf_decode", [out], "T = 0")
    _refused(L.tcavt_ltsf_front(d, d, d, d, d, d, out.ptr, out2.ptr, 1, 1, 8193, _st()), "ltsf_front", [out, out2], "T = 8193")
    _refused(L.tcavt_ltsf_front(d, d, d, d, d, None, out.ptr, out2.ptr, 1, 2, 2, _st()), "ltsf_front", [out, out2], "pos NULL")
    _refused(L.tcavt_ltsf_front(d, d, d, d, d, d, out.ptr, out2.ptr, 0, 2, 2, _st()), "ltsf_front", [out, out2], "B = 0")


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_transpose_ct, tcavt_out_head

@pytest.mark.parametrize("B,C,To", TRANSPOSE_CASES)
def test_transpose_ct(gpu, B, C, To):
    dev = gpu["device"]
    g_ = _gen(500 + B * C * To)
    v = _data((B, C, To), "realistic", g_) * torch.ldexp(torch.ones(B, C, 1), torch.randint(-12, 12, (B, C, 1), generator=g_)).double()
    src = _dev(v.reshape(B * C, To), dev)
    want = src.region.cpu().view(B, C, To).permute(0, 2, 1).reshape(B * To, C)
    for f32, dt in TRANSPOSE_OUTS:
        what = f"transpose_ct {(B, C, To)} fp32={f32} 16-bit={_name(dt) if dt else None}"
        of, ob = _twice(lambda of, ob: _L().tcavt_transpose_ct(src.buf.data_ptr(), _p(of), _p(ob), B, C, To, _dt_code(dt or BF16), _st()),
                        lambda: (_guarded(B * To, C, F32, dev) if f32 else None, _guarded(B * To, C, dt, dev) if dt else None),
                        _ins(**{"in": src}), what)
        if f32:
            _bits_equal(of.region, want, what + ": the fp32 output is not the transposed input")
        if dt:
            _bits_equal(ob.region, _round(want, dt), what + ": the 16-bit output is not the value rounded once")


def test_head_refusals(gpu):
    dev = gpu["device"]
    d = torch.zeros(64, device=dev).data_ptr()
    out = _guarded(4, 16, F32, dev)
    L = _L()
    _refused(L.tcavt_transpose_ct(d, None, None, 1, 4, 4, _dt_code(BF16), _st()), "transpose_ct", [out], "no output")
    _refused(L.tcavt_transpose_ct(d, out.ptr, None, 1, 4, 4, _dt_code(F32), _st()), "transpose_ct", [out], "dtype16 = TCAVT_F32")
    _refused(L.tcavt_transpose_ct(d, out.ptr, None, 1, 0, 4, _dt_code(BF16), _st()), "transpose_ct", [out], "C = 0")
    _refused(L.tcavt_poly_embed(d, d, d, d, None, 1, 2, 2, _st()), "poly_embed", [out], "x NULL")
    _refused(L.tcavt_poly_embed(d, d, d, d, out.ptr, 1, 0, 2, _st()), "poly_embed", [out], "P = 0")
    _refused(L.tcavt_masked_mean(d, None, out.ptr, 1, 2, 2, _st()), "masked_mean", [out], "len NULL")
    _refused(L.tcavt_masked_mean(d, d, out.ptr, 1, 2, 0, _st()), "masked_mean", [out], "D = 0")
    _refused(L.tcavt_out_head(d, d, d, None, out.ptr, 1, 2, 2, 2, 2, 0, _st()), "out_head", [out], "x NULL")
    _refused(L.tcavt_out_head(d, d, d, d, out.ptr, 1, 2, 2, 2, 0, 1, _st()), "out_head", [out], "T = 0")


@pytest.mark.parametrize("add_last", [0, 1])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("B,To,C,F,T", HEAD_CASES)
def test_out_head(gpu, B, To, C, F, T, regime, add_last):
    """out[b][f][s] = sum_c w[f][c] fused[b][s][c] + bias[f] (+ x[b][f][T - 1]): C chained fmaf, C E S with S = sum |w| |fused|, then
    two additions: 2 E (S + |bias| + |x_last|).  add_last == 0: x is all NaN and must not reach the output."""
    dev = gpu["device"]
    g_ = _gen(600 + B * To * C * F * T)
    fused, w, bias = _dev(_data((B * To, C), regime, g_), dev), _dev(_data((F, C), regime, g_, C ** -0.5), dev), _dev(_data((1, F), regime, g_), dev)
    xv = _data((B * F, T), regime, g_, 10.0)
    x = _dev(xv if add_last else torch.full_like(xv, float("nan")), dev)
    what = f"out_head {regime} {(B, To, C, F, T)} add_last={add_last}"
    (out,) = _twice(lambda out: _L().tcavt_out_head(fused.buf.data_ptr(), w.buf.data_ptr(), bias.buf.data_ptr(), x.buf.data_ptr(), out.ptr,
                                                   B, To, C, F, T, add_last, _st()),
                    lambda: (_guarded(B * F, To, F32, dev),), _ins(fused=fused, w=w, bias=bias, x=x), what)
    f64, w64, b64 = fused.region.double().cpu().view(B, To, C), w.region.double().cpu(), bias.region.double().cpu().view(F)
    xl = x.region.double().cpu().view(B, F, T)[:, :, -1:] if add_last else torch.zeros(B, F, 1, dtype=F64)
    acc = torch.einsum("fc,bsc->bfs", w64, f64)
    S = torch.einsum("fc,bsc->bfs", w64.abs(), f64.abs())
    ref = acc + b64[None, :, None] + xl
    rest = S + b64.abs()[None, :, None] + xl.abs()
    _judge(out.region.view(B, F, To), ref, C * _E * S + 2 * _E * rest, rest, regime, what, "tcavt_out_head")


def test_report_worst_ratio(gpu):
    """(runs last in file order) prints the worst fraction of the bound measured in this session per kernel"""
    for k in sorted(_WORST):
        print(f"{k:20s} f32   worst frac {_WORST[k]:7.3f}")
