"""The opt-in MX8 MLP on a real MI355X: tcavt_quant_mx8 and tcavt_gemm_mx8 against quant.py's definition and float64, the decoder
stage against its own composition from kernel-level calls, and the model switch.

Conventions of test_gemm_forms_gpu.py: outputs live inside larger poisoned buffers with padded leading dimensions (every
in-range element finite and correct, every other byte unchanged), inputs are bit-unchanged after the call, 16-bit side inputs and
outputs run in fp16 and bf16.  The codes' padding holds the e4m3 NaN code and the scales' padding 0xFF, so a read outside an
operand poisons the result.

1. lane map: exact one-hot data settles which k and which scale byte a lane's operand registers carry.
2. exact regime: integer codes in [-8, 8], block exponents in [-2, 3]; every partial sum is a multiple of 2^-4 below 2^20
   (asserted on |A| |W|^T), so the fp32 accumulator is exact in any order and every output is float64 plus one RNE rounding.
3. realistic regime: N(0, 1) * row gains through quant.quantize_mx; |got - ref| <= c * 2^-24 * (|Aq| |Wq|^T) * gain + epilogue ulps
   + ulp_out against the float64 product of the dequantised operands (_C_MX8 below).
"""
import ctypes
import math

import pytest
import torch

from test_gemm_forms_gpu import BF16, F16, F32, U, Poisoned, _WORST, _bits, _bound, _gemm, _round, _rs_eps
from tests.util import MODEL_CASES, batch_tensors, load_case, rel_err

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
# accumulator bar of the realistic regime: c in |got - ref| <= c * 2^-24 * (|Aq| |Wq|^T) * gain + ...  Worst c measured on an
# MI355X over every case of this module (test_report_worst_c, pytest -s): 266.4 (generic, fp16 side type, fp32 out; 260.5 with
# bf16; SiLU 243.0; NORM_OUT fp32 181.4; the 16-bit stream 95.6).  The constant is the smallest power of two >= 2 x worst; the
# margin covers run-to-run data, nothing else.  Against 1.13 for the 16-bit kernels this is a property of the instruction, not of
# the kernel around it ("MX8 MLP"): the 128 products of one v_mfma_scale are not added as a rounded fp32 chain.
_C_MX8 = 1024.0
NAN8, NANSC = 0x7F, 0xFF

SHAPES = [(1, 128, 128), (37, 256, 128), (300, 1152, 384), (520, 768, 1024), (2176, 2176, 256)]
SILU_SHAPES = [(512, 1024, 256), (300, 1152, 384)]
NORM_SHAPES = [(512, 256, 512), (300, 1152, 384), (1, 128, 128)]


def _capi():
    from tcavt_amd import capi

    return capi


def _dt_code(dt):
    capi = _capi()
    return {F32: capi.F32, BF16: capi.BF16, F16: capi.F16}[dt]


class PoisonedU8:
    """A uint8 [rows, cols] region inside a [rows + extra_rows, ld] buffer filled with `poison`."""

    def __init__(self, rows, cols, dev, ld, poison, extra_rows=3, fill=None):
        self.ld, self.rows, self.cols = ld, rows, cols
        self.buf = torch.full((rows + extra_rows, ld), poison, dtype=torch.uint8, device=dev)
        if fill is not None:
            self.buf[:rows, :cols] = fill.to(dev)
        self.before = self.buf.clone()

    @property
    def region(self):
        return self.buf[: self.rows, : self.cols]

    def check(self, what):
        out = torch.ones_like(self.buf, dtype=torch.bool)
        out[: self.rows, : self.cols] = False
        assert torch.equal(self.buf[out], self.before[out]), f"{what}: write outside [{self.rows}, {self.cols}]"

    def unchanged(self):
        return torch.equal(self.buf, self.before)


def _e4m3(vals):
    """uint8 codes of values that are e4m3 numbers"""
    c = vals.float().to(torch.float8_e4m3fn)
    assert torch.equal(c.double(), vals.double())
    return c.view(torch.uint8)


def _exps(shape, g):
    """block exponents in [-2, 3], the large ones rare (keeps the exact regime's sums inside the fp16 range)"""
    p = torch.tensor([0.3, 0.3, 0.2, 0.1, 0.05, 0.05])
    return (torch.multinomial(p, shape[0] * shape[1], replacement=True, generator=g).view(shape) - 2).to(torch.int32)


class Mx:
    """One MX8 operand in poisoned buffers: codes [R][K] (ld K + 64), scale bytes [R][K / 32] (ld K / 32 + 4), float64 values."""

    def __init__(self, codes, sb, dev):
        from tcavt_amd import quant

        R, K = codes.shape
        self.c = PoisonedU8(R, K, dev, K + 64, NAN8, fill=codes)
        self.s = PoisonedU8(R, K // 32, dev, K // 32 + 4, NANSC, fill=sb)
        self.val = quant.dequantize_mx(codes, sb, torch.float64).to(dev)


class Case:
    def __init__(self, M, N, K, dt, regime, seed, dev, gain=3.0):
        from tcavt_amd import quant

        g = torch.Generator().manual_seed(seed)
        self.M, self.N, self.K, self.dt, self.regime, self.dev, self.g = M, N, K, dt, regime, dev, g
        if regime == "exact":
            a = (_e4m3(torch.randint(-8, 9, (M, K), generator=g)), (_exps((M, K // 32), g) + 127).to(torch.uint8))
            w = (_e4m3(torch.randint(-8, 9, (N, K), generator=g)), (_exps((N, K // 32), g) + 127).to(torch.uint8))
        else:
            ga = torch.exp2((torch.rand(M, 1, generator=g) * 2 - 1) * gain)
            gw = torch.exp2((torch.rand(N, 1, generator=g) * 2 - 1) * gain)
            a = quant.quantize_mx((torch.randn(M, K, generator=g) * ga).to(dt))
            w = quant.quantize_mx((torch.randn(N, K, generator=g) / math.sqrt(K) * gw).to(dt))
        self.A, self.W = Mx(*a, dev), Mx(*w, dev)
        self.acc = self.A.val @ self.W.val.T
        self.abs = self.A.val.abs() @ self.W.val.abs().T
        if regime == "exact":
            assert self.abs.max().item() < 2.0 ** 20  # every partial sum, in any order, is a multiple of 2^-4 below 2^20

    def args(self, **kw):
        d = dict(A8=self.A.c.buf, lda=self.A.c.ld, A_scale=self.A.s.buf, ldsa=self.A.s.ld, W8=self.W.c.buf, ldw=self.W.c.ld,
                 W_scale=self.W.s.buf, ldsw=self.W.s.ld, M=self.M, N=self.N, K=self.K, dtype16=_dt_code(self.dt))
        d.update(kw)
        return d

    def check_inputs(self):
        for p, nm in ((self.A.c, "A8"), (self.A.s, "A_scale"), (self.W.c, "W8"), (self.W.s, "W_scale")):
            assert p.unchanged(), f"{nm} modified"

    def side(self, shape, scale=1.0, den=4):
        if self.regime == "exact":
            return (torch.randint(-8 * den, 8 * den + 1, shape, generator=self.g).float() / den).to(self.dev)
        return (torch.randn(shape, generator=self.g) * scale).to(self.dev)


def _mx8(**kw):
    """tcavt_gemm_mx8 with the given fields (tensors by pointer); returns the status code"""
    capi = _capi()
    a = capi.GemmMx8Args()
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
    rc = capi.lib().tcavt_gemm_mx8(ctypes.byref(a), capi.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _id(p):
    return "x".join(str(v) for v in p)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. lane map

@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("M", [16, 37, 48])
def test_lane_map(gpu, M, K):
    """One operand one-hot per row at column perm(row), the other distinct small integers (asymmetric), every (row, block) of both
    with its own exponent pattern in [-3, 3]: C must be the float64 product bit for bit.  Both roles (A one-hot, W one-hot).  A
    wrong k order, a swapped row / column or a wrong scale byte fails here.  (N = 128: the smallest the kernel takes; all 128 rows
    of W carry data.)"""
    dev = gpu["device"]
    capi = _capi()
    N = 128
    nb = K // 32

    def exps(R, a, b, c):
        r, blk = torch.arange(R)[:, None], torch.arange(nb)[None, :]
        return (((r * a + blk * b + c) % 7) - 3 + 127).to(torch.uint8)

    def onehot(R, mul, add):
        v = torch.zeros(R, K)
        v[torch.arange(R), (torch.arange(R) * mul + add) % K] = 1.0
        return v

    def ints(R, a, b):
        r, k = torch.arange(R)[:, None], torch.arange(K)[None, :]
        return (((r * a + k * b) % 17) - 8).float()

    for what, av, wv in (("A one-hot", onehot(M, 37, 11), ints(N, 7, 3)), ("W one-hot", ints(M, 5, 11), onehot(N, 29, 5))):
        A, W = Mx(_e4m3(av), exps(M, 3, 5, 0), dev), Mx(_e4m3(wv), exps(N, 5, 3, 1), dev)
        ref = A.val @ W.val.T
        assert len(torch.unique(ref)) > 20 and not torch.equal(ref[:, :M], ref[:, :M].T)
        C = Poisoned(M, N, F32, dev)
        rc = _mx8(A8=A.c.buf, lda=A.c.ld, A_scale=A.s.buf, ldsa=A.s.ld, W8=W.c.buf, ldw=W.c.ld, W_scale=W.s.buf, ldsw=W.s.ld,
                  M=M, N=N, K=K, dtype16=capi.F16, C=C.buf, ldc=C.ld, out_dtype=capi.F32)
        capi.check(rc, what)
        bad = _bits(C.region) != _bits(ref.float())
        assert not bool(bad.any()), f"lane map {what} {M}x{N}x{K}: {int(bad.sum())} differ, first {bad.nonzero()[0].tolist()}"
        C.check(what)


# ---------------------------------------------------------------------------------------------------------------------------
# 2 / 3. generic epilogue

@pytest.mark.parametrize("regime", ["exact", "real"])
@DTYPES
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_generic(gpu, shape, dt, regime):
    M, N, K = shape
    dev = gpu["device"]
    capi = _capi()
    cs = Case(M, N, K, dt, regime, seed=M * 31 + N + K, dev=dev)
    for out_dt in (F32, dt):
        what = f"mx8 generic {str(dt)[6:]}->{str(out_dt)[6:]} {regime}: {shape}"
        C = Poisoned(M, N, out_dt, dev)
        for rep in range(2):
            capi.check(_mx8(**cs.args(C=C.buf, ldc=C.ld, out_dtype=_dt_code(out_dt))), what)
            if rep == 0:
                first = C.buf.clone()
        assert torch.equal(_bits(first), _bits(C.buf)), f"{what}: two calls differ"
        if regime == "exact":
            want = _round(cs.acc, out_dt) if out_dt != F32 else cs.acc.float()
            bad = _bits(C.region) != _bits(want)
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ, first {bad.nonzero()[0].tolist()}"
        else:
            _bound(C.region, cs.acc, U * cs.abs, 0 * cs.acc, out_dt, what, c=_C_MX8)
        C.check(what)
        cs.check_inputs()


# ---------------------------------------------------------------------------------------------------------------------------
# SILU_MUL | ROWSCALE

@pytest.mark.parametrize("regime", ["exact", "real"])
@DTYPES
@pytest.mark.parametrize("shape", SILU_SHAPES, ids=_id)
def test_silu_mul(gpu, shape, dt, regime):
    """gate / up rows interleaved in blocks of 16; the existing SiLU bar (test_gemm_forms_gpu.test_silu_mul).  The exact regime's
    row scale is ~2^-9 so that the integer accumulators (thousands) give pre-activations of a few units."""
    M, N, K = shape
    I = N // 2
    dev = gpu["device"]
    capi = _capi()
    cs = Case(M, N, K, dt, regime, seed=M + 7 * N, dev=dev, gain=2.0)
    gate_rows = torch.tensor([(n // 16) % 2 == 0 for n in range(N)], device=dev)
    npart, h, eps = 32, 2048, 1e-5
    if regime == "exact":
        part = (torch.randint(1, 9, (M, npart), generator=cs.g).float() * (h / npart) * 4.0 ** 8).to(dev)
    else:
        part = (torch.rand(M, npart, generator=cs.g) * 2 * h / npart + 0.01).float().to(dev)
    rs = (1.0 / torch.sqrt(part.double().sum(1) / h + eps))[:, None]
    keep = part.clone()
    what = f"mx8 silu {str(dt)[6:]} {regime}: {shape}"
    C = Poisoned(M, I, dt, dev)
    rc = _mx8(**cs.args(C=C.buf, ldc=C.ld, out_dtype=_dt_code(dt), epilogue=capi.EPI_SILU_MUL | capi.EPI_ROWSCALE,
                        rowscale_part=part, rowscale_npart=npart, rowscale_h=h, rowscale_eps=eps))
    capi.check(rc, what)
    er = _rs_eps(npart)
    pre = cs.acc * rs
    gt, up = pre[:, gate_rows], pre[:, ~gate_rows]
    ag, au = cs.abs[:, gate_rows] * rs, cs.abs[:, ~gate_rows] * rs
    sg = torch.sigmoid(gt)
    ref = gt * sg * up
    dg, du = (sg * (1 + gt * (1 - sg)) * up).abs(), (gt * sg).abs()
    acc_unit = 0 * ref if regime == "exact" else U * (dg * ag + du * au)
    epi_err = (4 * U + er) * (dg * gt.abs() + du * up.abs()) + (8 + gt.abs()) * U * ref.abs()
    _bound(C.region, ref, acc_unit, epi_err, dt, what, c=_C_MX8)
    C.check(what)
    cs.check_inputs()
    assert torch.equal(part, keep)


# ---------------------------------------------------------------------------------------------------------------------------
# NORM_OUT: fp32 stream and the in-place 16-bit stream

@pytest.mark.parametrize("regime", ["exact", "real"])
@DTYPES
@pytest.mark.parametrize("shape", NORM_SHAPES, ids=_id)
def test_norm_out(gpu, shape, dt, regime):
    M, N, K = shape
    dev = gpu["device"]
    capi = _capi()
    cs = Case(M, N, K, dt, regime, seed=M + N * 5 + K, dev=dev, gain=2.0)
    npart, gw = N // 64, 64
    res = cs.side((M, N), scale=4.0, den=8)
    s16 = _round(cs.side((M, N), scale=4.0, den=8).double(), dt)
    keep_res, keep_s16 = res.clone(), s16.clone()
    flag = torch.zeros(4, dtype=torch.int32, device=dev)
    for mode in ("f32", "f32_res", "f32_res_ns", "s16", "s16_res", "s16_res_oop_ns"):
        what = f"mx8 norm {mode} {str(dt)[6:]} {regime}: {shape}"
        ns = 2.0 ** -3 if mode.endswith("_ns") else 1.0
        with_res = "res" in mode
        oop = "oop" in mode
        H = Poisoned(M, N, dt, dev, fill=s16 if mode.startswith("s16") and not oop else None)
        part = Poisoned(1, M * npart, F32, dev, ld=M * npart + 64, extra_rows=1)
        kw = dict(norm_h16=H.buf, norm_part=part.buf, norm_scale=ns if ns != 1.0 else 0.0, nonfinite_flag=flag, nonfinite_tag=7)
        epi = capi.EPI_NORM_OUT | (capi.EPI_RESIDUAL if with_res else 0)
        if mode.startswith("f32"):
            C = Poisoned(M, N, F32, dev)
            kw.update(C=C.buf, ldc=C.ld)
            if with_res:
                kw.update(residual=res, ldr=N)
        else:
            C = None
            kw.update(C=None, ldc=H.ld)
            if oop:
                src = Poisoned(M, N, dt, dev, ld=H.ld, fill=s16)
                kw.update(norm_res16=src.buf)
        capi.check(_mx8(**cs.args(out_dtype=capi.F32, epilogue=epi, **kw)), what)
        parts = part.buf[0, : M * npart].view(M, npart)
        if C is not None:
            ref = cs.acc + (res.double() if with_res else 0)
            if regime == "exact":
                assert torch.equal(_bits(C.region), _bits(ref.float())), f"{what}: C"
            else:
                _bound(C.region, ref, U * cs.abs, 2 * U * (cs.acc.abs() + res.double().abs()), F32, what, c=_C_MX8)
            C.check(what)
            v = C.region.double() * ns
            assert torch.equal(_bits(H.region), _bits(v.float().to(dt))), f"{what}: norm_h16 is not round(ns * C)"
            sq = v
        else:
            ref = ns * cs.acc + (s16.double() if with_res else 0)
            if regime == "exact":
                assert torch.equal(_bits(H.region), _bits(_round(ref, dt))), f"{what}: stream"
            else:
                _bound(H.region, ref, ns * U * cs.abs, 2 * U * ref.abs(), dt, what + " stream", c=_C_MX8)
            sq = H.region.double()
            if oop:
                assert torch.equal(_bits(src.buf), _bits(src.before)), f"{what}: norm_res16 modified"
        H.check(what + " h16")
        want = sq.view(M, npart, gw).pow(2).sum(-1)
        assert torch.isfinite(parts).all(), f"{what}: partial sums not all written"
        assert ((parts.double() - want).abs() <= (gw + 8) * U * want + 1e-30).all(), f"{what}: partial sums"
        part.check(what + " part")
        cs.check_inputs()
        assert torch.equal(res, keep_res) and torch.equal(s16, keep_s16)
    assert int(flag[0]) == 0, "nonfinite flag raised on finite data"
    # a planted inf in the 16-bit stream raises the flag with the caller's tag
    H = Poisoned(M, N, dt, dev, fill=s16)
    H.buf[M - 1, N - 1] = float("inf")
    part = torch.empty(M * npart, dtype=F32, device=dev)
    capi.check(_mx8(**cs.args(out_dtype=capi.F32, epilogue=capi.EPI_NORM_OUT | capi.EPI_RESIDUAL, C=None, ldc=H.ld, norm_h16=H.buf,
                              norm_part=part, nonfinite_flag=flag, nonfinite_tag=7)), "planted inf")
    assert int(flag[0]) == 7


def test_report_worst_c():
    """(pytest -s) worst accumulator ratio c per form over the realistic cases run so far"""
    for k in sorted(_WORST):
        if k.startswith("mx8"):
            print(f"[mx8 worst c] {k}: {_WORST[k]:.3f}")
    worst = max([v for k, v in _WORST.items() if k.startswith("mx8")], default=0.0)
    print(f"[mx8 worst c] overall {worst:.3f} (bar {_C_MX8})")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. quantise kernel

def _quant_input(M, K, dt, seed):
    from test_mx8_cpu import _wide

    x = _wide(dt, R=M, K=K, seed=seed)
    tiny = 2.0 ** -24 if dt == F16 else 2.0 ** -133
    # a zero block at the start of the matrix, then, in the first and the last row: amax exactly 448 * 2^j with two ties, one ulp
    # above it with 448 * 2^j at the block's other end, a subnormal block, a block at the smallest normal (bf16: below the clamp)
    x[0, :32] = 0
    x[0, 31] = -0.0
    ulp = 0.25 if dt == F16 else 2.0
    plant = [([448.0 / 64, 17.0 / 64] + [0.0] * 29 + [-19.0 / 64]), ([(448.0 + ulp) / 64] + [1.0 / 64] * 30 + [448.0 / 64]),
             [tiny] + [0.0] * 30 + [-3 * tiny], [2.0 ** -14 if dt == F16 else 2.0 ** -130] * 32]
    for i, vals in enumerate(plant):
        rr, bb = (M - 1, (K // 32 - 1 - i) % (K // 32)) if i % 2 else (0, (1 + i) % (K // 32))
        x[rr, 32 * bb: 32 * bb + 32] = torch.tensor(vals, dtype=torch.float64).to(dt)
    return x


@DTYPES
@pytest.mark.parametrize("K", [128, 1536])
@pytest.mark.parametrize("M", [1, 37, 300])
def test_quant_kernel_is_quantize_mx_byte_for_byte(gpu, M, K, dt):
    from tcavt_amd import capi, quant

    dev = gpu["device"]
    for nonfinite in (False, True):
        x = _quant_input(M, K, dt, seed=M + K)
        if nonfinite:
            x[M - 1, K - 1] = float("inf")
            x[0, 32 if K > 32 else 0] = float("nan")
            x[M // 2, K // 2] = -float("inf")
        X = Poisoned(M, K, dt, dev, ld=K + 64, extra_rows=3, fill=x)
        assert torch.equal(_bits(X.region.cpu()), _bits(x))
        codes = PoisonedU8(M, K, dev, K + 16, 0xA5)
        sb = PoisonedU8(M, K // 32, dev, K // 32 + 4, 0xA5)
        rc = capi.lib().tcavt_quant_mx8(X.buf.data_ptr(), X.ld, _dt_code(dt), codes.buf.data_ptr(), codes.ld, sb.buf.data_ptr(), sb.ld,
                                        M, K, capi.stream_ptr())
        torch.cuda.synchronize()
        capi.check(rc, "quant_mx8")
        wc, ws = quant.quantize_mx(x)
        bad = codes.region.cpu() != wc
        assert not bool(bad.any()), f"codes: {int(bad.sum())} differ, first {bad.nonzero()[0].tolist()}"
        bad = sb.region.cpu() != ws
        assert not bool(bad.any()), f"scale bytes: {int(bad.sum())} differ, first {bad.nonzero()[0].tolist()}"
        codes.check("codes")
        sb.check("scales")
        assert torch.equal(_bits(X.buf), _bits(X.before)), "input modified"


# ---------------------------------------------------------------------------------------------------------------------------
# 5. stage == composition

def _tiny_decoder(dev, storage, stream_scale):
    from tcavt_amd import config, model
    from tcavt_amd.weights import make_weights

    cfg = config.tiny(use_lora=True)
    m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(make_weights(cfg, 3), device=dev).eval()
    m.set_storage(storage, stream_scale=stream_scale)
    return cfg, m


def _prep(lw, x, M):
    from tcavt_amd import ops

    dev = x.device
    if lw.stream16:
        ops.rownorm_prep(x.clone(), *lw.norm_inputs(M, dev), npart=lw.norm_npart(M), rounded_sums=True, stream_scale=lw.stream_scale)
        return None
    h = x.clone()
    ops.rownorm_prep(h, *lw.norm_inputs(M, dev), npart=lw.norm_npart(M), stream_scale=lw.stream_scale)
    return h


def _compose(lw, h, kv_len, B, L, out):
    """tcavt_llama_stack_forward's launches for MX8 layers, issued one by one: today's entry points for the attention half,
    tcavt_quant_mx8 / tcavt_gemm_mx8 for the MLP half"""
    from tcavt_amd import capi, ops

    ll, P, dev = lw.shape, lw._prepared(), kv_len.device
    M, H, I, nq, nkv = B * L, ll.hidden, ll.inter, ll.n_q_heads, ll.n_kv_heads
    nqkv, dt, dtc = (nq + 2 * nkv) * 64, lw.storage, _dt_code(lw.storage)
    ss = lw.stream_scale
    eps_s = ll.rms_eps * ss * ss
    np_in, np_post = ops.norm_npart(M, H, I), ops.norm_npart(M, H, nq * 64)
    h16, part = lw.norm_inputs(M, dev)
    cos, sin = lw._rope_tables(L, dev)
    qkv = torch.empty(M, nqkv, dtype=dt, device=dev)
    att = torch.empty(M, nq * 64, dtype=dt, device=dev)
    act = torch.empty(M, I, dtype=dt, device=dev)
    t = torch.zeros(M, 64, dtype=dt, device=dev)
    stream16 = h is None
    MW = lw.mlp_weights("mx8")
    for li, d in enumerate(P.layers):
        ops.lora_down(h16, d.a_cat, t, lw.lora_alpha / lw.lora_r)
        capi.check(_gemm(A=h16, lda=H, W=d.w_qkv, ldw=H, C=qkv, ldc=nqkv, M=M, N=nqkv, K=H, out_dtype=dtc, in_dtype=dtc,
                         A2=t, lda2=64, W2=d.b_ext, ldw2=64, K2=64, epilogue=capi.EPI_ROPE | capi.EPI_ROWSCALE, rope_cos=cos,
                         rope_sin=sin, rope_L=L, rope_cols=(nq + nkv) * 64, rowscale_part=part, rowscale_npart=np_in, rowscale_h=H,
                         rowscale_eps=eps_s), "qkv")
        ops.attn_causal_gqa(qkv, att, kv_len, B, L, nq, nkv, 0.125)
        kw = dict(C=None, norm_h16=h16, norm_res16=h16) if stream16 else dict(C=h, residual=h, ldr=H, norm_h16=h16)
        capi.check(_gemm(A=att, lda=nq * 64, W=d.w_o, ldw=nq * 64, ldc=H, M=M, N=H, K=nq * 64, out_dtype=capi.F32, in_dtype=dtc,
                         epilogue=capi.EPI_RESIDUAL | capi.EPI_NORM_OUT, norm_part=part, norm_scale=ss, **kw), "o")
        (gu8, gus), (d8, ds) = MW.keep[li]
        c8, s8 = ops.quant_mx8(h16)
        ops.gemm_mx8(c8, s8, gu8, gus, act, dt, epilogue=capi.EPI_SILU_MUL | capi.EPI_ROWSCALE, rowscale_part=part,
                     rowscale_npart=np_post, rowscale_h=H, rowscale_eps=eps_s)
        c8, s8 = ops.quant_mx8(act)
        if stream16:
            ops.gemm_mx8(c8, s8, d8, ds, None, dt, epilogue=capi.EPI_RESIDUAL | capi.EPI_NORM_OUT, ldc=H, norm_h16=h16,
                         norm_res16=h16, norm_part=part, norm_scale=ss)
        else:
            ops.gemm_mx8(c8, s8, d8, ds, h, dt, epilogue=capi.EPI_RESIDUAL | capi.EPI_NORM_OUT, residual=h, ldr=H, norm_h16=h16,
                         norm_part=part, norm_scale=ss)
    if stream16:
        ops.rmsnorm16(h16, P.g_final, eps_s, out_f32=out)
    else:
        ops.rmsnorm(h, P.g_final, ll.rms_eps, out_f32=out)
    torch.cuda.synchronize()


@pytest.mark.parametrize("storage,stream_scale", [(F16, 1.0), (F16, 0.25), (BF16, 1.0)], ids=["f16", "f16_scaled", "bf16_f32stream"])
def test_stage_equals_composition(gpu, storage, stream_scale):
    dev = gpu["device"]
    cfg, m = _tiny_decoder(dev, storage, stream_scale)
    lw = m.mllm.llama_wrapper
    assert lw.stream16 == (storage == F16)
    B, L = 3, 40
    M, H = B * L, lw.shape.hidden
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, H, generator=g).to(dev)
    kv_len = torch.tensor([40, 33, 17], dtype=torch.int32, device=dev)
    outs = {}
    with torch.no_grad():
        for prec in ("mx8", "fp16"):
            m.set_mlp_precision(prec)
            out = torch.full((M, H), float("nan"), device=dev)
            h = _prep(lw, x, M)
            # (decoder_stack hands o_proj its split-K workspace; at K = 256 the host rule takes one launch, as _compose does)
            lw.decoder_stack(h, kv_len, B, L, out_f32=out)
            torch.cuda.synchronize()
            outs[prec] = out
        m.set_mlp_precision("mx8")
        comp = torch.full((M, H), float("nan"), device=dev)
        _compose(lw, _prep(lw, x, M), kv_len, B, L, comp)
    assert torch.isfinite(outs["mx8"]).all()
    assert torch.equal(_bits(outs["mx8"]), _bits(comp)), "stage differs from its composition"
    assert not torch.equal(outs["mx8"], outs["fp16"])  # (the MX8 layers did run)
    assert rel_err(outs["mx8"], outs["fp16"]) < 0.1


# ---------------------------------------------------------------------------------------------------------------------------
# 6 / 7. the model switch

def _fwd(m, g, with_loss=True):
    kw = dict(input_ids=g["input_ids"], attention_mask=g["attention_mask"], labels=g["labels"])
    if with_loss:
        kw.update(y=g["target_traj"], norm_stat=g["norm_stat"])
    return m(g["traj_emb"], g["vision_emb"], None, g["lane_polygon"], g["lane_polygon_len"], **kw)


def _model(dev, name, weights=None):
    from tcavt_amd import model

    cfg, w, fx = load_case(name)
    m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights or w, device=dev).eval()
    return cfg, m, fx, {k: v.to(dev) for k, v in batch_tensors(fx).items()}


def test_off_means_off(gpu):
    dev = gpu["device"]
    cfg, m, fx, g = _model(dev, "tiny_6_12_lora_ragged")
    _, ref_m, _, _ = _model(dev, "tiny_6_12_lora_ragged")
    with torch.no_grad():
        loss0, dec0 = _fwd(ref_m, g)
        m.set_mlp_precision("mx8")
        loss8, dec8 = _fwd(m, g)
        fh8 = m.last.final_hidden.clone()
        m.set_mlp_precision("fp16")
        loss1, dec1 = _fwd(m, g)
        torch.cuda.synchronize()
    m.mllm.check_flags()
    assert torch.equal(dec1, dec0) and torch.equal(loss1, loss0) and torch.equal(m.last.final_hidden, ref_m.last.final_hidden)
    assert torch.isfinite(dec8).all() and not torch.equal(fh8, m.last.final_hidden)
    assert m.mllm.llama_wrapper._prep_mx8 is not None
    m.invalidate_prepared()
    assert m.mllm.llama_wrapper._prep_mx8 is None


def test_overflow_in_the_mx8_down_projection_is_flagged(gpu):
    import numpy as np

    from tcavt_amd.weights import LLAMA_PREFIX

    dev = gpu["device"]
    cfg, w, fx = load_case("tiny_6_12_lora_ragged")
    w = dict(w)
    for k, sc in ((f"{LLAMA_PREFIX}layers.0.mlp.down_proj.weight", 2e4), (f"{LLAMA_PREFIX}layers.0.mlp.up_proj.weight", 1e3)):
        w[k] = w[k] * np.float32(sc)
    cfg, m, fx, g = _model(dev, "tiny_6_12_lora_ragged", weights=w)
    m.set_mlp_precision("mx8")
    with torch.no_grad():
        loss, dec = _fwd(m, g)
        torch.cuda.synchronize()
    assert not torch.isfinite(loss.float()).all()
    with pytest.raises(FloatingPointError, match="down_proj epilogue of layer 0"):
        m.mllm.check_flags()


def test_mx8_with_a_tape_raises(gpu):
    from tcavt_amd import capi

    dev = gpu["device"]
    cfg, m, fx, g = _model(dev, "tiny_6_12_lora_ragged")
    m.set_mlp_precision("mx8")
    lw = m.mllm.llama_wrapper
    lw.save_for_backward = True
    with torch.no_grad(), pytest.raises(capi.TcavtError, match="cannot run with a tape"):
        _fwd(m, g)
    lw.save_for_backward = False
    torch.cuda.synchronize()


def test_hipgraph_replay_of_an_mx8_pass_equals_eager(gpu):
    dev = gpu["device"]
    cfg, m, fx, g = _model(dev, "tiny_18_30_nolora_ragged")
    m.set_mlp_precision("mx8")
    static = {k: v.clone() for k, v in g.items()}
    with torch.no_grad():
        for _ in range(2):
            _fwd(m, static)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            _fwd(m, static)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g_loss, g_dec = _fwd(m, static)
        static["vision_emb"].copy_(g["vision_emb"] * 0.9 + 0.05)
        graph.replay()
        torch.cuda.synchronize()
        got_loss, got_dec = g_loss.clone(), g_dec.clone()
        e_loss, e_dec = _fwd(m, {k: v.clone() for k, v in static.items()})
        torch.cuda.synchronize()
    assert torch.equal(got_dec, e_dec) and torch.equal(got_loss, e_loss), "hipGraph replay of the MX8 pass differs from eager"
    m.mllm.check_flags()


# Deviation of the MX8 path from the REFERENCE's own fp32 outputs (the fixture arrays), relative L2.  No bound can be derived for a
# 2-layer tiny model: measured once on an MI355X (fp16 storage), each bar 2 x the measured value; the margin covers the other
# fixtures and dtypes.  (The fp16 path's own figures on these fixtures: decoded ~2e-4, final_hidden ~1e-3.)
#                name: (decoded bar, final_hidden bar)            measured: decoded / final_hidden
_DEVIATION = {
    "tiny_6_12_lora_ragged": (2 * 5.390e-03, 2 * 2.968e-02),     # 5.390e-03 / 2.968e-02
    "tiny_18_30_nolora_ragged": (2 * 4.209e-03, 2 * 3.710e-02),  # 4.209e-03 / 3.710e-02
    "tiny_6_30_lora_full": (2 * 3.241e-03, 2 * 2.889e-02),       # 3.241e-03 / 2.889e-02
}


@pytest.mark.parametrize("name", MODEL_CASES)
def test_model_deviation_from_the_reference(gpu, name):
    dev = gpu["device"]
    cfg, m, fx, g = _model(dev, name)
    m.set_mlp_precision("mx8")
    with torch.no_grad():
        loss, dec = _fwd(m, g)
        torch.cuda.synchronize()
    m.mllm.check_flags()
    e_dec, e_fh = rel_err(dec.cpu(), fx["exp_decoded"]), rel_err(m.last.final_hidden.cpu(), fx["exp_final_hidden"])
    print(f"[mx8 deviation {name}] decoded {e_dec:.3e}  final_hidden {e_fh:.3e}  (vs the reference's fp32 outputs)")
    bar_dec, bar_fh = _DEVIATION[name]
    assert e_dec <= bar_dec and e_fh <= bar_fh
