"""tcavt_gemm_bf16 form by form against float64, in fp16 and bf16, with poisoned buffers.

Every case calls the C entry point through capi.GemmArgs and checks it against torch.matmul in float64 on the GPU, the
epilogue evaluated in float64 from the same fp32 side inputs.  Two operand regimes:

- exact: small-integer operands, every fp32 partial sum an integer below 2^24, so the accumulator is exact in any
  summation order.  The generic epilogue (fp32 out, integer / dyadic bias and residual, acc_scale a power of two), every
  16-bit output (one RNE rounding of an exact value), NORM_OUT's C and 16-bit copy and the NORM16 stream must then equal
  the reference bit for bit.  SiLU and RoPE keep only their fp32 epilogue error (a few ulps, see the bounds).
- realistic: N(0, 1)-scaled operands, each element within  c * 2^-24 * (|A| |W|^T)_ij * gain + epilogue ulps + ulp_out(ref).
  The worst measured c over the module is written next to each bar (_C_ACC).

Outputs (C, silu_preact, norm_h16, norm_part) live inside larger NaN-filled buffers (ldc = n_out + 16, two extra rows):
every in-range element must be finite and correct, every other element keep its bits.  A, W, A2 and W2 have a leading
dimension of K + 64 with NaN in the padding and NaN rows after M and N.  A, W, bias, a residual C does not alias, the
row-scale partials, the cos / sin tables and the positions must be bit-unchanged after the call.

Coverage (form: how it is reached -- shapes M x N x K; gx = XCD partition of the tile grid, _gx() mirrors the host rule):

| form | reached by | generic | SiLU (+ROWSCALE, +preact) | RoPE (+ROWSCALE, +K2, rope_pos) | NORM / NORM16 |
|---|---|---|---|---|---|
| 64x64 PIPE 2 | tile 64 | 300x208x256 | 300x1152x256 | (tile 64 runs 128x128) | refused |
| 128x128 PIPE 2 (<= 256 WGs) | tile 128 | 300x208 (gx 8); 2048x1024 (gx 4); 1024x4096 (gx 2); 512x8192 (gx 1) | 300x1152 | 300x768 | 300x576 |
| 128x128 PIPE 1 (> 256 WGs) | tile 128 | 2100x2064 (gx 8); 4096x2048 (gx 4); 2048x4096 (gx 2); 1024x16384 (gx 1) | 2100x2176 | 2100x2176 (+K2) | 2100x2112 |
| 8-wave 256x256 | tile 256 | 520x784 (gx 8); 4096x2048 (gx 4); 2048x4096 (gx 2); 1024x8192 (gx 1) | 520x1152 | 520x768 (+K2) | 520x832 |
| 4-wave 256x256 | tile 257 | 512x768 (K2 refused); 4096x4608 persistent | 512x768; 4096x4608 | 512x768 (+K2) | 512x512; 4096x4608 |
| 4-wave deep | tile 272 | 512x768; 4096x4608 | 512x768; 4096x4608 | (runs 257) | 512x512; 4096x4608 |
| 4-wave 256x192 | tile 271 | 512x768; 4352x3072 persistent | 512x768 | 512x768; 4352x3072 (+K2, rope_cols 2560) | 512x768 |
| skinny | tile 0, M <= 32, K % 256 | M 1, 17, 32 x 512; 32x8192 (two column blocks) | 17x1024 (no preact) | 17x768 (K2 = 64) | 17x512 |
| two-launch split K | tile 0, NORM16, workspace | | | | 1024x2048x4096 |
| SILU_BWD | tile 0 / 257 | 512x512x256 in place and out of place | | | |
| batched (batch > 1), dropout epilogue | tiles 0, 64, 128, 256 | tests/test_gemm_batched_gpu.py, same rules and helpers | | | |

Each row runs in bf16 and fp16 and in both regimes; out dtypes f32 and the operand type (the 4-wave SiLU / RoPE forms
refuse f32, asserted).  test_decoder_projections runs the four projections with tcavt_llama_stack_forward's flag sets at
the 1B shape (M = 8192, 6400, 1024).  test_tile_codes_bit_identical, the fp16-range tests and test_gx_coverage cover
the claims of gemm_bf16.hip and DESIGN section 2.
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
U = 2.0 ** -24
# accumulator bar: c in |got - ref| <= c * 2^-24 * (|A| |W|^T) * gain + ...  (K = 128 .. 8192 here).  Measured on an MI355X:
# worst 1.13 (generic, tile 272, bf16 operands, fp32 out); 1.9 for BIAS_ROW while its rounding was still charged to the
# accumulator.  test_report_worst_ratio prints the worst c per form (pytest -s)
_C_ACC = 4.0
_WORST = {}


def _lib():
    from tcavt_amd import capi

    return capi


def _dt_code(dt):
    capi = _lib()
    return {F32: capi.F32, BF16: capi.BF16, F16: capi.F16}[dt]


def _gemm(**kw):
    """tcavt_gemm_bf16 with the given GemmArgs fields (tensors are passed by pointer); returns the status code."""
    capi = _lib()
    a = capi.GemmArgs()
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
    rc = capi.lib().tcavt_gemm_bf16(ctypes.byref(a), capi.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _bits(t):
    return t.view({F32: torch.int32, F16: torch.int16, BF16: torch.int16, torch.int32: torch.int32}[t.dtype])


def _ulp(x, dt):
    """ulp of dt at |x| (float64 tensor), subnormal spacing below the normal range"""
    p, emin = {F16: (10, -14), BF16: (7, -126), F32: (23, -126)}[dt]
    _, e = torch.frexp(x)
    e = torch.where(x == 0, torch.full_like(e, emin + 1), e)
    return torch.ldexp(torch.ones_like(x), (e - 1).clamp_min(emin) - p)


class Poisoned:
    """A [rows, cols] region inside a NaN-filled [rows + extra_rows, ld] buffer; .region is the view to pass, .check() asserts
    that nothing outside the region changed."""

    def __init__(self, rows, cols, dt, dev, ld=None, extra_rows=2, fill=None):
        self.ld = cols + 16 if ld is None else ld
        self.buf = torch.full((rows + extra_rows, self.ld), float("nan"), dtype=dt, device=dev)
        self.rows, self.cols = rows, cols
        if fill is not None:
            self.buf[:rows, :cols] = fill.to(dt)
        self.before = self.buf.clone()

    @property
    def region(self):
        return self.buf[: self.rows, : self.cols]

    def check(self, what):
        out = torch.ones_like(self.buf, dtype=torch.bool)
        out[: self.rows, : self.cols] = False
        assert torch.equal(_bits(self.buf)[out], _bits(self.before)[out]), f"{what}: write outside [{self.rows}, {self.cols}]"


def _ints(shape, r, g):
    return torch.randint(-r, r + 1, shape, generator=g).double()


def _operand(rows, K, dt, dev, vals):
    """vals [rows, K] in a buffer with lda = K + 64, NaN padding and three NaN rows after the last one"""
    return Poisoned(rows, K, dt, dev, ld=K + 64, extra_rows=3, fill=vals)


class Case:
    """Operands of one product C = A W^T (+ A2 W2^T) in poisoned buffers, their float64 product and |A| |W|^T."""

    def __init__(self, M, N, K, dt, regime, seed, dev, K2=0, r=None, w_rows=None):
        g = torch.Generator().manual_seed(seed)
        self.M, self.N, self.K, self.K2, self.dt, self.regime, self.dev = M, N, K, K2, dt, regime, dev
        if regime == "exact":
            r = r if r is not None else (4 if K + K2 <= 2048 else 2)
            a, w = _ints((M, K), r, g), _ints((N, K), r, g) if w_rows is None else w_rows
            a2, w2 = (_ints((M, K2), r, g), _ints((N, K2), r, g)) if K2 else (None, None)
        else:
            a = torch.randn(M, K, generator=g).double()
            w = (torch.randn(N, K, generator=g) / math.sqrt(K)).double() if w_rows is None else w_rows
            a2 = torch.randn(M, K2, generator=g).double() if K2 else None
            w2 = (torch.randn(N, K2, generator=g) / math.sqrt(K2)).double() if K2 else None
        self.g = g
        self.pA, self.pW = _operand(M, K, dt, dev, a), _operand(N, K, dt, dev, w)
        self.pA2 = _operand(M, K2, dt, dev, a2) if K2 else None
        self.pW2 = _operand(N, K2, dt, dev, w2) if K2 else None
        A64, W64 = self.pA.region.double(), self.pW.region.double()
        self.acc = A64 @ W64.T
        self.abs = A64.abs() @ W64.abs().T
        if K2:
            A2, W2 = self.pA2.region.double(), self.pW2.region.double()
            self.acc += A2 @ W2.T
            self.abs += A2.abs() @ W2.abs().T

    def args(self, tile, **kw):
        d = dict(A=self.pA.buf, lda=self.pA.ld, W=self.pW.buf, ldw=self.pW.ld, M=self.M, N=self.N, K=self.K, tile=tile,
                 in_dtype=_dt_code(self.dt))
        if self.K2:
            d.update(A2=self.pA2.buf, lda2=self.pA2.ld, W2=self.pW2.buf, ldw2=self.pW2.ld, K2=self.K2)
        d.update(kw)
        return d

    def check_inputs(self):
        for p, nm in ((self.pA, "A"), (self.pW, "W"), (self.pA2, "A2"), (self.pW2, "W2")):
            if p is not None:
                assert torch.equal(_bits(p.buf), _bits(p.before)), f"{nm} modified"

    def side(self, shape, scale=1.0, den=4):
        """fp32 side input: dyadic small numbers in the exact regime, N(0, scale^2) otherwise"""
        if self.regime == "exact":
            return (torch.randint(-8 * den, 8 * den + 1, shape, generator=self.g).float() / den).to(self.dev)
        return (torch.randn(shape, generator=self.g) * scale).to(self.dev)


def _bound(got, ref, acc_unit, epi_err, out_dt, what, c=None):
    """|got - ref| <= c * acc_unit + epi_err + ulp_out(ref), elementwise; every element finite.  acc_unit = 0 in the exact regime."""
    c = _C_ACC if c is None else c
    g = got.double()
    assert torch.isfinite(g).all(), f"{what}: {int((~torch.isfinite(g)).sum())} non-finite in range (unwritten tile?)"
    d = (g - ref).abs()
    slack = d - epi_err - _ulp(ref, out_dt)
    bad = slack > c * acc_unit
    if bool(bad.any()):
        idx = bad.nonzero()[0].tolist()
        i = tuple(idx)
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of bound; first {i}: got {g[i].item()!r} ref {ref[i].item()!r} "
                             f"allowed {(c * acc_unit + epi_err + _ulp(ref, out_dt))[i].item():.3e}")
    pos = acc_unit > 0
    if bool(pos.any()):
        worst = (slack[pos] / acc_unit[pos]).max().item()
        _WORST[what.split(":")[0]] = max(_WORST.get(what.split(":")[0], 0.0), worst)


def _round(ref, dt):
    """one RNE rounding of an fp32-exact value into dt"""
    return ref.float().to(dt)


# ---------------------------------------------------------------------------------------------------------------------------
# host-rule mirrors

def _gx(M, N, K, BM, BN):
    """choose_xcd_partition (gemm_bf16.hip) for a BM x BN tile grid"""
    tm, tn = -(-M // BM), -(-N // BN)
    a, w = M * K, N * K
    best, cost = 8, a + 8.0 * w
    for gx in (4, 2, 1):
        gy = 8 // gx
        if tm % gx or tn % gy or (tm // gx) % 4 or (tm * tn) % 8:
            continue
        c = gy * a + gx * w
        if c < cost:
            best, cost = gx, c
    return best


def _form(tile, M, N, epi="generic"):
    """kernel form a forced tile code runs (launch_small / dispatch_tile)"""
    if tile == 64 and epi not in ("rope", "norm"):
        return "64"
    if tile in (64, 128):
        return "128p2" if -(-M // 128) * -(-N // 128) <= 256 else "128p1"
    return {256: "256", 257: "257", 272: "272" if epi != "rope" else "257", 271: "271", 0: "auto"}[tile]


GENERIC_SHAPES = [  # (tile, M, N, K)
    (64, 300, 208, 256),
    (128, 300, 208, 256), (128, 2048, 1024, 128), (128, 1024, 4096, 128), (128, 512, 8192, 128),
    (128, 2100, 2064, 128), (128, 4096, 2048, 128), (128, 2048, 4096, 128), (128, 1024, 16384, 128),
    (256, 520, 784, 256), (256, 4096, 2048, 128), (256, 2048, 4096, 128), (256, 1024, 8192, 128),
    (257, 512, 768, 256), (257, 4096, 4608, 128), (272, 512, 768, 256), (272, 4096, 4608, 128),
    (271, 512, 768, 256), (271, 4352, 3072, 128),
    (0, 1, 512, 512), (0, 17, 512, 512), (0, 32, 512, 512), (0, 32, 8192, 256),
]


def test_gx_coverage():
    """the shape list reaches every XCD partition gx in {1, 2, 4, 8} for the 128x128 forms (both PIPEs) and the 8-wave form"""
    seen = {}
    for tile, M, N, K in GENERIC_SHAPES:
        if tile in (128, 256):
            bm = 128 if tile == 128 else 256
            seen.setdefault(_form(tile, M, N), set()).add(_gx(M, N, K, bm, bm))
    for f in ("128p2", "128p1", "256"):
        assert seen[f] == {1, 2, 4, 8}, (f, seen.get(f))
    assert _gx(2100, 2064, 128, 128, 128) == 8 and _form(128, 2100, 2064) == "128p1"  # 289 tiles, both edges partial


def _id(p):
    return "x".join(str(v) for v in p)


# ---------------------------------------------------------------------------------------------------------------------------
# generic epilogue

def _accepts_generic(tile, M, N, K2, out_dt, dt):
    if tile in (257, 272, 271) and K2:
        return False  # the 4-wave kernel takes a second K source for RoPE only
    return True


@pytest.mark.parametrize("regime", ["exact", "real"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", GENERIC_SHAPES, ids=_id)
def test_generic(gpu, shape, dt, regime):
    tile, M, N, K = shape
    dev = gpu["device"]
    capi = _lib()
    cs = Case(M, N, K, dt, regime, seed=M * 31 + N + K + tile, dev=dev)
    cs2 = Case(M, N, K, dt, regime, seed=M * 31 + N + K + tile + 1, dev=dev, K2=64) if tile != 0 else None
    bias, brow, res = cs.side((N,)), cs.side((M,)), cs.side((M, N), scale=4.0, den=8)
    keep = [t.clone() for t in (bias, brow, res)]
    variants = [("plain", {}, 0), ("bias", dict(bias=bias), capi.EPI_BIAS),
                ("bias_relu", dict(bias=bias), capi.EPI_BIAS | capi.EPI_RELU),
                ("res", dict(residual=res, ldr=N), capi.EPI_RESIDUAL), ("bias_row", dict(bias=brow), capi.EPI_BIAS_ROW),
                ("scale", dict(acc_scale=0.25), 0), ("res_inplace", {}, capi.EPI_RESIDUAL), ("k2", {}, 0)]
    for out_dt in (F32, dt):
        for name, kw, epi in variants:
            c = cs2 if name == "k2" else cs
            if c is None:
                continue
            if name == "res_inplace" and out_dt != F32:
                continue
            what = f"generic {_form(tile, M, N)} {name} {str(dt)[6:]}->{str(out_dt)[6:]} {regime}: {shape}"
            C = Poisoned(M, N, out_dt, dev, fill=res if name == "res_inplace" else None)
            if name == "res_inplace":
                kw = dict(residual=C.buf, ldr=C.ld)
            rc = _gemm(**c.args(tile, C=C.buf, ldc=C.ld, out_dtype=_dt_code(out_dt), epilogue=epi, **kw))
            if not _accepts_generic(tile, M, N, c.K2, out_dt, dt):
                assert rc != 0, f"{what}: accepted"
                assert torch.equal(_bits(C.buf), _bits(C.before)), f"{what}: refused call wrote"
                continue
            capi.check(rc, what)
            s = kw.get("acc_scale", 1.0)
            ref = c.acc * s
            if epi & capi.EPI_BIAS:
                ref = ref + bias.double()
            if epi & capi.EPI_BIAS_ROW:
                ref = ref + brow.double()[:, None]
            if epi & capi.EPI_RELU:
                ref = ref.clamp_min(0)
            mag = ref.abs() + (bias.double().abs() if epi & capi.EPI_BIAS else 0) + (brow.double().abs()[:, None] if epi & capi.EPI_BIAS_ROW else 0)
            if epi & capi.EPI_RESIDUAL:
                ref = ref + res.double()
                mag = mag + res.double().abs()
            got = C.region
            if regime == "exact":
                want = _round(ref, out_dt) if out_dt != F32 else ref.float()
                bad = _bits(got) != _bits(want)
                assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ, first {bad.nonzero()[0].tolist()}"
            else:
                _bound(got, ref, s * U * c.abs, 4 * U * mag, out_dt, what)
            C.check(what)
            c.check_inputs()
    for t, k in zip((bias, brow, res), keep):
        assert torch.equal(t, k)


# ---------------------------------------------------------------------------------------------------------------------------
# shared pieces of the transcendental epilogues

def _rowscale(cs, npart, h=2048, eps=1e-5):
    """fp32 partial sums [M, npart] and the float64 row scale the kernel applies (partials added in index order)"""
    M = cs.M
    if cs.regime == "exact":
        part = (torch.randint(1, 9, (M, npart), generator=cs.g).float() * (h / npart)).to(cs.dev)  # mean in [1, 8]
    else:
        part = (torch.rand(M, npart, generator=cs.g) * 2 * h / npart + 0.01).float().to(cs.dev)
    rs = 1.0 / torch.sqrt(part.double().sum(1) / h + eps)
    return part, rs[:, None], dict(rowscale_part=part, rowscale_npart=npart, rowscale_h=h, rowscale_eps=eps)


def _rs_eps(npart):
    return (npart + 8) * U  # relative error of the kernel's row scale: fp32 sum of npart partials, rsqrtf


SILU_SHAPES = [  # (tile, M, N, K): N = 2 I, interleaved gate|up
    (64, 300, 1152, 256), (128, 300, 1152, 256), (128, 2100, 2176, 128), (256, 520, 1152, 256),
    (257, 512, 768, 256), (257, 4096, 4608, 128), (272, 512, 768, 256), (272, 4096, 4608, 128), (271, 512, 768, 256),
    (0, 17, 1024, 256),
]


@pytest.mark.parametrize("regime", ["exact", "real"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", SILU_SHAPES, ids=_id)
def test_silu_mul(gpu, shape, dt, regime):
    from tcavt_amd.layout import interleave_gate_up

    tile, M, N, K = shape
    I = N // 2
    dev = gpu["device"]
    capi = _lib()
    g = torch.Generator().manual_seed(N + K + M)
    if regime == "exact":
        wg, wu = _ints((I, K), 1, g), _ints((I, K), 1, g)
    else:
        wg, wu = torch.randn(I, K, generator=g).double() / math.sqrt(K), torch.randn(I, K, generator=g).double() / math.sqrt(K)
    w = interleave_gate_up(wg, wu)
    cs = Case(M, N, K, dt, regime, seed=M + 7 * N, dev=dev, r=1, w_rows=w)
    gate_rows = torch.tensor([(n // 16) % 2 == 0 for n in range(N)], device=dev)
    # the interleaved layout: gate feature f at row 32 (f // 16) + f % 16, up feature f 16 rows further on
    assert torch.equal(cs.pW.region[gate_rows].cpu(), wg.to(dt)) and torch.equal(cs.pW.region[~gate_rows].cpu(), wu.to(dt))
    npart = 32
    part, rs, rskw = _rowscale(cs, npart)
    keep = part.clone()
    for out_dt in (dt, F32) if tile else (dt,):
        for rowscale in (False, True):
            for save in (False, True):
                if tile == 0 and save:
                    continue  # (the skinny form takes no silu_preact: tile 0 runs the 64x64 form, covered above)
                what = f"silu {_form(tile, M, N)} rs={int(rowscale)} save={int(save)} {str(dt)[6:]}->{str(out_dt)[6:]} {regime}: {shape}"
                C = Poisoned(M, I, out_dt, dev)
                P = Poisoned(M, N, dt, dev) if save else None
                kw = dict(rskw) if rowscale else {}
                if save:
                    kw.update(silu_preact=P.buf, ld_preact=P.ld)
                epi = capi.EPI_SILU_MUL | (capi.EPI_ROWSCALE if rowscale else 0)
                rc = _gemm(**cs.args(tile, C=C.buf, ldc=C.ld, out_dtype=_dt_code(out_dt), epilogue=epi, **kw))
                if out_dt == F32 and tile in (257, 271, 272):
                    assert rc != 0, f"{what}: accepted"  # the 4-wave SiLU epilogue writes the operand type only
                    C.check(what)
                    continue
                capi.check(rc, what)
                r = rs if rowscale else torch.ones_like(rs)
                er = _rs_eps(npart) if rowscale else 0.0
                pre = cs.acc * r
                gt, up = pre[:, gate_rows], pre[:, ~gate_rows]
                ag, au = cs.abs[:, gate_rows] * r, cs.abs[:, ~gate_rows] * r
                sg = torch.sigmoid(gt)
                ref = gt * sg * up
                dg, du = (sg * (1 + gt * (1 - sg)) * up).abs(), (gt * sg).abs()
                acc_unit = 0 * ref if regime == "exact" else U * (dg * ag + du * au)
                epi_err = (4 * U + er) * (dg * gt.abs() + du * up.abs()) + (8 + gt.abs()) * U * ref.abs()
                _bound(C.region, ref, acc_unit, epi_err, out_dt, what)
                C.check(what)
                if save:
                    pun = cs.abs * r
                    if regime == "exact" and not rowscale:
                        assert torch.equal(_bits(P.region), _bits(_round(pre, dt))), f"{what}: preact"
                    else:
                        _bound(P.region, pre, 0 * pre if regime == "exact" else U * pun, (2 * U + er) * pre.abs(), dt, what + " preact")
                    P.check(what + " preact")
                cs.check_inputs()
    assert torch.equal(part, keep)


# ---------------------------------------------------------------------------------------------------------------------------
# RoPE

def _rope_tables(L, dev):
    inv = 1.0 / (10000.0 ** (torch.arange(0, 64, 2, dtype=torch.float64) / 64))
    ang = torch.arange(L, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().float().contiguous().to(dev), ang.sin().float().contiguous().to(dev)


def _rope_ref(x, cos, sin, pos, rope_cols):
    """half-split RoPE (head_dim 64) on columns [0, rope_cols) of x [M, N] (float64); returns out, |c|-weighted pieces"""
    M, N = x.shape
    c, s = cos.double()[pos], sin.double()[pos]  # [M, 32]
    h = x.view(M, N // 64, 2, 32)
    lo, hi = h[:, :, 0], h[:, :, 1]
    rot = rope_cols // 64
    out = h.clone()
    out[:, :rot, 0] = lo[:, :rot] * c[:, None] - hi[:, :rot] * s[:, None]
    out[:, :rot, 1] = hi[:, :rot] * c[:, None] + lo[:, :rot] * s[:, None]
    return out.view(M, N), c, s


def _rope_err(v, a, c, s, rope_cols):
    """|d out| for accumulator errors a (per element of x) and rounding magnitudes: mixes the two halves as the rotation does"""
    M, N = v.shape
    rot = rope_cols // 64
    hv, ha = v.view(M, N // 64, 2, 32), a.view(M, N // 64, 2, 32)
    mag, unit = hv.abs().clone(), ha.clone()
    ca, sa = c.abs()[:, None], s.abs()[:, None]
    for half in (0, 1):
        mag[:, :rot, half] = hv[:, :rot, 0].abs() * (ca if half == 0 else sa) + hv[:, :rot, 1].abs() * (sa if half == 0 else ca)
        unit[:, :rot, half] = ha[:, :rot, 0] * (ca if half == 0 else sa) + ha[:, :rot, 1] * (sa if half == 0 else ca)
    return mag.view(M, N), unit.view(M, N)


ROPE_SHAPES = [  # (tile, M, N, K, rope_cols): rope_cols ends inside a 192-wide tile
    (128, 300, 768, 256, 640), (128, 2100, 2176, 128, 1984), (256, 520, 768, 256, 640), (257, 512, 768, 256, 640),
    (271, 512, 768, 256, 640), (271, 4352, 3072, 128, 2560), (0, 17, 768, 256, 640),
]


@pytest.mark.parametrize("regime", ["exact", "real"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", ROPE_SHAPES, ids=_id)
def test_rope(gpu, shape, dt, regime):
    tile, M, N, K, rope_cols = shape
    dev = gpu["device"]
    capi = _lib()
    L = 40
    cos, sin = _rope_tables(300, dev)
    cos_l, sin_l = cos[:L].contiguous(), sin[:L].contiguous()
    g = torch.Generator().manual_seed(M + N)
    pos = torch.randint(0, 300, (M,), generator=g, dtype=torch.int32).to(dev)
    cases = {0: Case(M, N, K, dt, regime, seed=M * 3 + N, dev=dev), 64: Case(M, N, K, dt, regime, seed=M * 3 + N + 1, dev=dev, K2=64)}
    npart = 32
    part, rs, rskw = _rowscale(cases[0], npart)
    keep = [t.clone() for t in (cos, sin, cos_l, sin_l, pos, part)]
    for out_dt in (dt, F32) if tile else (dt,):
        for rowscale, K2, use_pos in ((False, 0, False), (True, 0, False), (True, 64, False), (True, 64, True), (False, 64, True)):
            cs = cases[K2]
            what = (f"rope {_form(tile, M, N, 'rope')} rs={int(rowscale)} K2={K2} pos={int(use_pos)} {str(dt)[6:]}->{str(out_dt)[6:]} "
                    f"{regime}: {shape}")
            C = Poisoned(M, N, out_dt, dev)
            kw = dict(rskw) if rowscale else {}
            if use_pos:
                kw.update(rope_cos=cos, rope_sin=sin, rope_L=300, rope_pos=pos)
            else:
                kw.update(rope_cos=cos_l, rope_sin=sin_l, rope_L=L)
            epi = capi.EPI_ROPE | (capi.EPI_ROWSCALE if rowscale else 0)
            rc = _gemm(**cs.args(tile, C=C.buf, ldc=C.ld, out_dtype=_dt_code(out_dt), epilogue=epi, rope_cols=rope_cols, **kw))
            if out_dt == F32 and tile in (257, 271):
                assert rc != 0, f"{what}: accepted"  # the 4-wave RoPE epilogue writes the operand type only
                C.check(what)
                continue
            capi.check(rc, what)
            r = rs if rowscale else torch.ones_like(rs)
            er = _rs_eps(npart) if rowscale else 0.0
            x = cs.acc * r
            p = pos.long() if use_pos else torch.arange(M, device=dev) % L
            ref, c, s = _rope_ref(x, cos, sin, p, rope_cols)
            mag, unit = _rope_err(x, cs.abs * r, c, s, rope_cols)
            acc_unit = 0 * ref if regime == "exact" else U * unit
            _bound(C.region, ref, acc_unit, (6 * U + er) * mag, out_dt, what)
            C.check(what)
            cs.check_inputs()
    for t, k in zip((cos, sin, cos_l, sin_l, pos, part), keep):
        assert torch.equal(t, k)


# ---------------------------------------------------------------------------------------------------------------------------
# NORM_OUT: fp32 stream (C, norm_h16 copy, partial sums of squares) and the 16-bit stream (C == NULL)

NORM_SHAPES = [  # (tile, M, N, K): N % 64 == 0
    (128, 300, 576, 256), (128, 2100, 2112, 128), (256, 520, 832, 256), (257, 512, 512, 256), (257, 4096, 4608, 128),
    (272, 512, 512, 256), (272, 4096, 4608, 128), (271, 512, 768, 256), (0, 17, 512, 256),
]


def _npart(tile, M, N, K):
    from tcavt_amd import ops

    return ops.norm_npart(M, N, K) if tile == 0 else N // 64


@pytest.mark.parametrize("regime", ["exact", "real"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", NORM_SHAPES, ids=_id)
def test_norm_out(gpu, shape, dt, regime):
    tile, M, N, K = shape
    dev = gpu["device"]
    capi = _lib()
    cs = Case(M, N, K, dt, regime, seed=M + N * 5 + K, dev=dev)
    npart = _npart(tile, M, N, K)
    gw = N // npart
    res = cs.side((M, N), scale=4.0, den=8)
    s16 = _round(cs.side((M, N), scale=4.0, den=8).double(), dt)
    keep_res, keep_s16 = res.clone(), s16.clone()
    flag = torch.zeros(4, dtype=torch.int32, device=dev)
    for mode in ("f32", "f32_res", "f32_res_ns", "s16", "s16_res", "s16_res_oop", "s16_res_ns"):
        what = f"norm {_form(tile, M, N, 'norm')} {mode} {str(dt)[6:]} {regime}: {shape}"
        ns = 2.0 ** -3 if mode.endswith("_ns") else 1.0
        with_res = "res" in mode
        H = Poisoned(M, N, dt, dev, fill=s16 if mode.startswith("s16") and mode != "s16_res_oop" else None)
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
            if mode == "s16_res_oop":
                src = Poisoned(M, N, dt, dev, ld=H.ld, fill=s16)
                kw.update(norm_res16=src.buf)
        rc = _gemm(**cs.args(tile, out_dtype=capi.F32, epilogue=epi, **kw))
        capi.check(rc, what)
        parts = part.buf[0, : M * npart].view(M, npart)
        if C is not None:
            ref = cs.acc + (res.double() if with_res else 0)
            if regime == "exact":
                assert torch.equal(_bits(C.region), _bits(ref.float())), f"{what}: C"
            else:
                _bound(C.region, ref, U * cs.abs, 2 * U * (cs.acc.abs() + res.double().abs()), F32, what)
            C.check(what)
            v = C.region.double() * ns  # what the kernel rounds: its own fp32 result at the stream scale
            assert torch.equal(_bits(H.region), _bits(v.float().to(dt))), f"{what}: norm_h16 is not round(ns * C)"
            sq = v
        else:
            ref = ns * cs.acc + (s16.double() if with_res else 0)
            if regime == "exact":
                assert torch.equal(_bits(H.region), _bits(_round(ref, dt))), f"{what}: stream"
            else:
                _bound(H.region, ref, ns * U * cs.abs, 2 * U * ref.abs(), dt, what + " stream")
            sq = H.region.double()  # partial sums of the ROUNDED values
            if mode == "s16_res_oop":
                assert torch.equal(_bits(src.buf), _bits(src.before)), f"{what}: norm_res16 modified"
        H.check(what + " h16")
        want = sq.view(M, npart, gw).pow(2).sum(-1)
        assert torch.isfinite(parts).all(), f"{what}: partial sums not all written"
        assert ((parts.double() - want).abs() <= (gw + 8) * U * want + 1e-30).all(), f"{what}: partial sums"
        part.check(what + " part")
        cs.check_inputs()
        assert torch.equal(res, keep_res) and torch.equal(s16, keep_s16)
    assert int(flag[0]) == 0, "nonfinite flag raised on finite data"


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_norm16_two_launch_split_k(gpu, dt):
    """tile 0, NORM16 with a workspace on a small grid: S partial products into fp32 slabs + a reduce.  The slab region past the
    first 16 KiB holds garbage: the result must be finite and correct, and a second run over other garbage bit-equal."""
    dev = gpu["device"]
    capi = _lib()
    M, N, K = 1024, 2048, 4096
    for regime in ("exact", "real"):
        cs = Case(M, N, K, dt, regime, seed=K + N, dev=dev)
        s16 = _round(cs.side((M, N), scale=4.0, den=8).double(), dt)
        ws = torch.zeros((16 << 10) + 8 * M * N * 4, dtype=torch.uint8, device=dev)
        outs = []
        for garbage in (0xFF, 0x7F):  # NaN, then 3.4e38
            ws[16 << 10:] = garbage
            H = Poisoned(M, N, dt, dev, fill=s16)
            part = torch.full((M * (N // 64) + 64,), float("nan"), device=dev)
            rc = _gemm(**cs.args(0, C=None, ldc=H.ld, out_dtype=capi.F32, epilogue=capi.EPI_NORM_OUT | capi.EPI_RESIDUAL,
                                 norm_h16=H.buf, norm_part=part, splitk_ws=ws, splitk_ws_bytes=ws.numel()))
            capi.check(rc, "split-K")
            assert torch.equal(ws[: 16 << 10], torch.zeros(16 << 10, dtype=torch.uint8, device=dev)), "tickets not left zero"
            assert not torch.equal(ws[16 << 10: (16 << 10) + 64], torch.full((64,), garbage, dtype=torch.uint8, device=dev)), \
                "the slabs were not used: no split"
            ref = cs.acc + s16.double()
            what = f"splitk {str(dt)[6:]} {regime}"
            if regime == "exact":
                assert torch.equal(_bits(H.region), _bits(_round(ref, dt))), what
            else:
                _bound(H.region, ref, U * cs.abs, 2 * U * ref.abs(), dt, what)
            H.check(what)
            assert torch.isnan(part[M * (N // 64):]).all()
            want = H.region.double().view(M, N // 64, 64).pow(2).sum(-1)
            got = part[: M * (N // 64)].view(M, N // 64).double()
            assert ((got - want).abs() <= 72 * U * want).all(), what
            outs.append((H.region.clone(), got.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "depends on the slab garbage"


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_silu_bwd(gpu, dt):
    """SILU_BWD (4-wave only): d(gate|up) from the accumulator d = g . w_t^T and the interleaved pre-activations, in place and
    out of place"""
    dev = gpu["device"]
    capi = _lib()
    M, I, H = 512, 512, 256
    for regime in ("exact", "real"):
        cs = Case(M, I, H, dt, regime, seed=I + H, dev=dev, r=1)
        g = torch.Generator().manual_seed(3)
        pre = (torch.randn(M, 2 * I, generator=g) * 2).to(dt).to(dev)
        gate_cols = torch.tensor([(n // 16) % 2 == 0 for n in range(2 * I)], device=dev)
        gt, up = pre[:, gate_cols].double(), pre[:, ~gate_cols].double()
        sg = torch.sigmoid(gt)
        d = cs.acc
        ref = torch.empty(M, 2 * I, dtype=torch.float64, device=dev)
        ref[:, gate_cols] = d * up * sg * (1 + gt * (1 - sg))
        ref[:, ~gate_cols] = d * gt * sg
        ad = 0 * d if regime == "exact" else U * cs.abs
        unit = torch.empty_like(ref)
        unit[:, gate_cols] = ad * (up * sg * (1 + gt * (1 - sg))).abs()
        unit[:, ~gate_cols] = ad * (gt * sg).abs()
        mag = torch.empty_like(ref)
        mag[:, gate_cols] = (16 + gt.abs()) * U * (d * up).abs() * (1 + gt.abs())
        mag[:, ~gate_cols] = (16 + gt.abs()) * U * (d * gt).abs()
        for inplace in (True, False):
            what = f"silu_bwd {str(dt)[6:]} {regime} inplace={int(inplace)}"
            P = Poisoned(M, 2 * I, dt, dev, fill=pre)
            C = P if inplace else Poisoned(M, 2 * I, dt, dev)
            rc = _gemm(**cs.args(0, C=C.buf, ldc=C.ld, out_dtype=_dt_code(dt), epilogue=capi.EPI_SILU_BWD, silu_preact=P.buf,
                                 ld_preact=P.ld))
            capi.check(rc, what)
            _bound(C.region, ref, unit, mag, dt, what)
            C.check(what)
            if not inplace:
                assert torch.equal(_bits(P.buf), _bits(P.before)), f"{what}: silu_preact modified"
            cs.check_inputs()


# ---------------------------------------------------------------------------------------------------------------------------
# the decoder's own calls (tcavt_llama_stack_forward, 16-bit residual stream), fp16 at the 1B shape, tile 0

@pytest.mark.parametrize("regime", ["exact", "real"])
@pytest.mark.parametrize("M", [8192, 6400, 1024])
def test_decoder_projections(gpu, M, regime):
    dev = gpu["device"]
    capi = _lib()
    dt, H, I, nq, nkv = F16, 2048, 8192, 32, 8
    L = 256 if M == 8192 else (200 if M == 6400 else 128)
    nqkv = (nq + 2 * nkv) * 64
    eps = 1e-5
    npart = H // 64
    cos, sin = _rope_tables(L, dev)
    ws = torch.zeros((16 << 10) + 8 * 1024 * 2048 * 4, dtype=torch.uint8, device=dev) if M == 1024 else None
    # q|k|v: ROPE | ROWSCALE with the LoRA second K source (t [M, 64] . b_ext [N, 64]^T)
    cs = Case(M, nqkv, H, dt, regime, seed=M + 1, dev=dev, K2=64, r=2)
    part, rs, rskw = _rowscale(cs, npart, h=H, eps=eps)
    C = Poisoned(M, nqkv, dt, dev)
    rc = _gemm(**cs.args(0, C=C.buf, ldc=C.ld, out_dtype=capi.F16, epilogue=capi.EPI_ROPE | capi.EPI_ROWSCALE, rope_cos=cos,
                         rope_sin=sin, rope_L=L, rope_cols=(nq + nkv) * 64, **rskw))
    capi.check(rc, "q|k|v")
    x = cs.acc * rs
    ref, c, s = _rope_ref(x, cos, sin, torch.arange(M, device=dev) % L, (nq + nkv) * 64)
    mag, unit = _rope_err(x, cs.abs * rs, c, s, (nq + nkv) * 64)
    _bound(C.region, ref, 0 * ref if regime == "exact" else U * unit, (6 * U + _rs_eps(npart)) * mag, dt, f"decoder qkv {regime}: {M}")
    C.check("q|k|v")
    cs.check_inputs()
    del cs, C, ref, mag, unit, x
    # o: h16 += att . W_o^T in place, partial sums for the post-attention norm
    for name, K, N in (("o", nq * 64, H), ("down", I, H)):
        cs = Case(M, N, K, dt, regime, seed=M + K, dev=dev)
        s16 = _round(cs.side((M, N), scale=4.0, den=8).double(), dt)
        Hs = Poisoned(M, N, dt, dev, fill=s16)
        pt = torch.full((M * npart + 64,), float("nan"), device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        kw = dict(splitk_ws=ws, splitk_ws_bytes=ws.numel()) if ws is not None else {}
        rc = _gemm(**cs.args(0, C=None, ldc=Hs.ld, out_dtype=capi.F32, epilogue=capi.EPI_NORM_OUT | capi.EPI_RESIDUAL,
                             norm_h16=Hs.buf, norm_part=pt, nonfinite_flag=flag, nonfinite_tag=3, **kw))
        capi.check(rc, name)
        ref = cs.acc + s16.double()
        what = f"decoder {name} {regime}: {M}"
        if regime == "exact":
            assert torch.equal(_bits(Hs.region), _bits(_round(ref, dt))), what
        else:
            _bound(Hs.region, ref, U * cs.abs, 2 * U * ref.abs(), dt, what)
        Hs.check(what)
        want = Hs.region.double().view(M, npart, 64).pow(2).sum(-1)
        assert ((pt[: M * npart].view(M, npart).double() - want).abs() <= 72 * U * want).all(), what
        assert torch.isnan(pt[M * npart:]).all() and int(flag) == 0
        cs.check_inputs()
        del cs, Hs, ref, want
    # gate|up: SILU_MUL | ROWSCALE
    cs = Case(M, 2 * I, H, dt, regime, seed=M + 2, dev=dev, r=1)
    part, rs, rskw = _rowscale(cs, npart, h=H, eps=eps)
    C = Poisoned(M, I, dt, dev)
    rc = _gemm(**cs.args(0, C=C.buf, ldc=C.ld, out_dtype=capi.F16, epilogue=capi.EPI_SILU_MUL | capi.EPI_ROWSCALE, **rskw))
    capi.check(rc, "gate|up")
    gate_rows = (torch.arange(2 * I, device=dev) // 16) % 2 == 0
    pre = cs.acc * rs
    gt, up = pre[:, gate_rows], pre[:, ~gate_rows]
    sg = torch.sigmoid(gt)
    ref = gt * sg * up
    dg, du = (sg * (1 + gt * (1 - sg)) * up).abs(), (gt * sg).abs()
    acc_unit = 0 * ref if regime == "exact" else U * (dg * cs.abs[:, gate_rows] * rs + du * cs.abs[:, ~gate_rows] * rs)
    epi_err = (4 * U + _rs_eps(npart)) * (dg * gt.abs() + du * up.abs()) + (8 + gt.abs()) * U * ref.abs()
    _bound(C.region, ref, acc_unit, epi_err, dt, f"decoder gate|up {regime}: {M}")
    C.check("gate|up")
    cs.check_inputs()


# ---------------------------------------------------------------------------------------------------------------------------
# claims: bit identity across tile codes; fp16 range on every 16-bit store path

@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_tile_codes_bit_identical(gpu, dt):
    """tcavt_gemm_args.tile: 64, 128, 256, 257, 271 and 272 give bit-identical results (one shape all of them accept)"""
    dev = gpu["device"]
    capi = _lib()
    M, N, K = 512, 768, 256
    cs = Case(M, N, K, dt, "real", seed=11, dev=dev)
    cs2 = Case(M, N, K, dt, "real", seed=12, dev=dev, K2=64)
    res = cs.side((M, N))
    bias = cs.side((N,))
    part, _, rskw = _rowscale(cs, 32)
    cos, sin = _rope_tables(64, dev)
    forms = {
        "generic16": (cs, dict(out_dtype=_dt_code(dt), epilogue=0), (M, N, dt), (64, 128, 256, 257, 271, 272)),
        "generic32_bias_relu_res": (cs, dict(out_dtype=capi.F32, epilogue=capi.EPI_BIAS | capi.EPI_RELU | capi.EPI_RESIDUAL,
                                             bias=bias, residual=res, ldr=N), (M, N, F32), (64, 128, 256, 257, 271, 272)),
        "silu_rs": (cs, dict(out_dtype=_dt_code(dt), epilogue=capi.EPI_SILU_MUL | capi.EPI_ROWSCALE, **rskw), (M, N // 2, dt),
                    (64, 128, 256, 257, 271, 272)),
        "rope_rs_k2": (cs2, dict(out_dtype=_dt_code(dt), epilogue=capi.EPI_ROPE | capi.EPI_ROWSCALE, rope_cos=cos, rope_sin=sin,
                                 rope_L=64, rope_cols=640, **rskw), (M, N, dt), (64, 128, 256, 257, 271, 272)),
        "norm32_res": (cs, dict(out_dtype=capi.F32, epilogue=capi.EPI_NORM_OUT | capi.EPI_RESIDUAL, residual=res, ldr=N),
                       (M, N, F32), (128, 256, 257, 271, 272)),
        "norm16_res": (cs, dict(out_dtype=capi.F32, epilogue=capi.EPI_NORM_OUT | capi.EPI_RESIDUAL, C=None),
                       (M, N, dt), (128, 256, 257, 271, 272)),
    }
    s16 = res.to(dt)
    for name, (c, kw, (r, n, odt), tiles) in forms.items():
        outs = {}
        for tile in tiles:
            kw2 = dict(kw)
            if name.startswith("norm"):
                h = s16.clone() if name == "norm16_res" else torch.zeros(M, N, dtype=dt, device=dev)
                pt = torch.zeros(M, N // 64, device=dev)
                kw2.update(norm_h16=h, norm_part=pt)
            if name == "norm16_res":
                out = h
                kw2.update(ldc=N)
            else:
                out = torch.zeros(r, n, dtype=odt, device=dev)
                kw2.update(C=out, ldc=n)
            capi.check(_gemm(**c.args(tile, **kw2)), f"{name} tile {tile}")
            outs[tile] = [out] + ([h, pt] if name.startswith("norm") else [])
        for tile in tiles:
            for a, b in zip(outs[tile], outs[256]):
                assert torch.equal(_bits(a), _bits(b)), (name, tile)
    # tile 64 refuses NORM_OUT (its waves cover 32 columns: no whole 64-column group)
    h = torch.zeros(M, N, dtype=dt, device=dev)
    assert _gemm(**cs.args(64, C=None, ldc=N, out_dtype=capi.F32, epilogue=capi.EPI_NORM_OUT, norm_h16=h,
                           norm_part=torch.zeros(M, N // 64, device=dev))) != 0


RANGE_FORMS = [(128, 300, 256), (257, 512, 512)]  # general path (partial tiles) and a whole-tile fast path


@pytest.mark.parametrize("tile,M,N", RANGE_FORMS, ids=["128-partial", "257-whole"])
def test_fp16_overflow_is_inf(gpu, tile, M, N):
    """|value| > 65504 stores +-inf on every 16-bit store path, never a clamped 65504; NORM / NORM16 raise
    nonfinite_flag with their tag while the fp32 C stays finite"""
    dev = gpu["device"]
    capi = _lib()
    K = 128
    a = torch.full((M, K), 4.0, dtype=F16, device=dev)
    a[1::2] = -4.0  # odd rows negative
    w = torch.full((N, K), 160.0, dtype=F16, device=dev)  # acc = +-81920
    base = dict(A=a, lda=K, W=w, ldw=K, M=M, N=N, K=K, tile=tile, in_dtype=capi.F16)
    sign = torch.where(torch.arange(M, device=dev) % 2 == 0, 1.0, -1.0)[:, None]

    def is_inf(t, s):
        return bool((t.float() == s * float("inf")).all())

    C = torch.zeros(M, N, dtype=F16, device=dev)
    capi.check(_gemm(**base, C=C, ldc=N, out_dtype=capi.F16), "generic")
    assert is_inf(C, sign.expand(M, N)), "generic"
    res = torch.zeros(M, N, device=dev)
    C.zero_()
    capi.check(_gemm(**base, C=C, ldc=N, out_dtype=capi.F16, residual=res, ldr=N, epilogue=capi.EPI_RESIDUAL), "generic+res")
    assert is_inf(C, sign.expand(M, N)), "generic general path"
    S = torch.zeros(M, N // 2, dtype=F16, device=dev)
    capi.check(_gemm(**base, C=S, ldc=N // 2, out_dtype=capi.F16, epilogue=capi.EPI_SILU_MUL), "silu")
    # silu(g) * u with g = u = 81920: +inf; with g = u = -81920: silu(g) = -0 * ... = -0 (a finite zero)
    assert is_inf(S[0::2], 1.0) and bool((S[1::2].float() == 0).all()), "silu"
    cos, sin = torch.ones(4, 32, device=dev), torch.zeros(4, 32, device=dev)
    R = torch.zeros(M, N, dtype=F16, device=dev)
    capi.check(_gemm(**base, C=R, ldc=N, out_dtype=capi.F16, epilogue=capi.EPI_ROPE, rope_cos=cos, rope_sin=sin, rope_L=4,
                     rope_cols=128), "rope")
    assert is_inf(R, sign.expand(M, N)), "rope"
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    Cf, h, pt = torch.zeros(M, N, device=dev), torch.zeros(M, N, dtype=F16, device=dev), torch.zeros(M, N // 64, device=dev)
    capi.check(_gemm(**base, C=Cf, ldc=N, out_dtype=capi.F32, epilogue=capi.EPI_NORM_OUT, norm_h16=h, norm_part=pt,
                     nonfinite_flag=flag, nonfinite_tag=5), "norm")
    assert torch.isfinite(Cf).all() and bool((Cf.abs() == 81920).all()) and is_inf(h, sign.expand(M, N)), "norm copy"
    assert int(flag) == 5, "norm: nonfinite_flag not raised"
    flag.zero_()
    h = torch.zeros(M, N, dtype=F16, device=dev)
    capi.check(_gemm(**base, C=None, ldc=N, out_dtype=capi.F32, epilogue=capi.EPI_NORM_OUT | capi.EPI_RESIDUAL, norm_h16=h,
                     norm_part=pt, nonfinite_flag=flag, nonfinite_tag=9), "norm16")
    assert is_inf(h, sign.expand(M, N)) and int(flag) == 9, "norm16 stream"


def test_fp16_subnormals_nan_relu(gpu):
    """a result in fp16's subnormal range is stored as torch rounds it (not flushed); subnormal fp16 operands multiply exactly;
    a NaN in A comes through RELU as NaN"""
    dev = gpu["device"]
    capi = _lib()
    M, N, K = 300, 208, 128
    g = torch.Generator().manual_seed(1)
    # subnormal results: normal operands 2^-12 * small integers, sums of size 2^-24 .. 2^-15
    a = (torch.randint(-3, 4, (M, K), generator=g).double() * 2.0 ** -12).to(F16).to(dev)
    w = (torch.randint(-3, 4, (N, K), generator=g).double() * 2.0 ** -12).to(F16).to(dev)
    ref = a.double() @ w.double().T
    for tile in (128, 256):
        P = Poisoned(M, N, F16, dev)
        capi.check(_gemm(A=a, lda=K, W=w, ldw=K, C=P.buf, ldc=P.ld, M=M, N=N, K=K, tile=tile, in_dtype=capi.F16, out_dtype=capi.F16), "sub")
        C = P.region
        assert torch.equal(_bits(C), _bits(ref.float().to(F16))), f"subnormal results, tile {tile}"
        assert bool((C != 0).any()) and bool((C.abs() < 2.0 ** -14).any())
        P.check("subnormal results")
    # subnormal operands: 2^-20 * small integers (fp16 subnormals) times 2^4 * integers
    a = (torch.randint(-3, 4, (M, K), generator=g).double() * 2.0 ** -20).to(F16).to(dev)
    w = (torch.randint(-3, 4, (N, K), generator=g).double() * 16).to(F16).to(dev)
    assert bool((a != 0).any()) and bool((a.abs() < 2.0 ** -14).all())
    P = Poisoned(M, N, F32, dev)
    capi.check(_gemm(A=a, lda=K, W=w, ldw=K, C=P.buf, ldc=P.ld, M=M, N=N, K=K, tile=128, in_dtype=capi.F16, out_dtype=capi.F32), "subop")
    assert torch.equal(P.region, (a.double() @ w.double().T).float()), "subnormal fp16 operands are not multiplied exactly"
    P.check("subnormal operands")
    # NaN through RELU
    a = torch.randn(M, K, generator=g).to(F16).to(dev)
    a[5, 7] = float("nan")
    w = torch.randn(N, K, generator=g).to(F16).to(dev)
    bias = torch.zeros(N, device=dev)
    for out_dt in (F32, F16):
        P = Poisoned(M, N, out_dt, dev)
        capi.check(_gemm(A=a, lda=K, W=w, ldw=K, C=P.buf, ldc=P.ld, M=M, N=N, K=K, tile=128, in_dtype=capi.F16,
                         out_dtype=_dt_code(out_dt), bias=bias, epilogue=capi.EPI_BIAS | capi.EPI_RELU), "relu")
        C = P.region
        assert torch.isnan(C[5]).all() and torch.isfinite(C[torch.arange(M, device=dev) != 5]).all()
        P.check("relu")


def test_report_worst_ratio(gpu):
    """(runs last in file order) prints the worst accumulator ratio c measured per form in this session"""
    for k in sorted(_WORST):
        print(f"worst c  {k:60s} {_WORST[k]:.3f}")
