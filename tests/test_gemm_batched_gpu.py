"""tcavt_gemm_bf16's batched form and its dropout epilogue against float64, element by element, with poisoned buffers.

The two parts of the entry point that tests/test_gemm_forms_gpu.py leaves out, under that module's rules and with its helpers
(Poisoned, _bits, _ulp, _ints, _bound, _round, _gemm, the bar _C_ACC): an exact regime (small-integer operands, dyadic side
inputs: the output is the float64 reference rounded once, bit for bit) and a realistic one (N(0, 1) operands, every element
within  _C_ACC * 2^-24 * (|A| |W|^T) * gain + 4 * 2^-24 * mag + ulp_out(ref)).

Batched form.  tests/gemm_batched_ref.py holds the call sites' stride patterns and the strided float64 reference (proven on
the CPU by tests/test_gemm_batched_ref_cpu.py).  A, W and C are flat buffers; operand elements no product addresses are NaN,
C starts as NaN everywhere.  After the call every addressed C element is finite and within bound, every other element of C
keeps its bits, and A, W, bias and residual keep theirs.  Every case runs fp16 and bf16 operands, fp32 and operand-type
outputs, both regimes, and the four tile codes that accept a batch, whose results must be bit-identical.  Forms reached
(_batched_form mirrors tcavt_gemm_bf16's tile choice and launch_small, which count the batch):

| case | M x N x K, batch / inner / w_group | tile 0 | tile 64 | tile 128 | tile 256 |
|---|---|---|---|---|---|
| xattn_scores (+ shared bias / residual) | 30x128x128, 6 / 2 / 1 | 64x64 | 64x64 | 128x128 PIPE 2 | 8-wave |
| xattn_pv | 30x128x128, 6 / 2 / 1 | 64x64 | 64x64 | 128x128 PIPE 2 | 8-wave |
| v_transposed (BIAS_ROW) | 128x64x128, 3 / 1 / 1 | 64x64 | 64x64 | 128x128 PIPE 2 | 8-wave |
| absorbed_scores | 30x128x256, 6 / 2 / 1 | 64x64 | 64x64 | 128x128 PIPE 2 | 8-wave |
| gqa_scores (w_group 2, 4 = inner, 0) | 40x64x64, 8 / 4 | 64x64 | 64x64 | 128x128 PIPE 2 | 8-wave |
| gqa_dq (w_group 2, 4 = inner, 0), gqa_dk_block | 40x64x64, 8 / 4 | 64x64 | 64x64 | 128x128 PIPE 2 | 8-wave |
| pipe1_batch96 | 256x256x64, 96 / 8 / 1 | 128x128 PIPE 1 (384 workgroups) | 64x64 | 128x128 PIPE 1 | 8-wave |
| skinny_shaped | 17x48x256, 6 / 2 / 1 | 64x64 (not the skinny form: batch > 1) | 64x64 | 128x128 PIPE 2 | 8-wave |
| max_batch | 16x16x64, 65535 / 1 / 1 | 8-wave (65535 tiles fill whole waves) | 64x64 | 128x128 PIPE 1 | 8-wave |

Dropout epilogue (EPI_DROP: its own instantiations).  The keep mask is oracle.philox.keep_mask over the flat index m * N + n,
C has ldc = N + 16; order bias, ReLU, dropout, residual.  Forms reached (_drop_form mirrors the dispatch: tile codes other
than 64 and 128 are served as tile 0):

| shape | tile 64 | tile 128 | tile 0 | tile 256 |
|---|---|---|---|---|
| 300x208x256 | 64x64 | 128x128 PIPE 2 | 64x64 (6 workgroups) | 64x64 (served as tile 0) |
| 2100x2064x128 | | 128x128 PIPE 1 (289 workgroups, both edges partial) | | |

test_report_worst_ratio (pytest -s) prints the worst accumulator ratio c per case; profiles/gemm_batched_bounds.txt holds a run.
"""
import functools

import pytest
import torch

from tests import gemm_batched_ref as R
from tests import test_gemm_forms_gpu as GF

pytestmark = pytest.mark.gpu

F16, BF16, F32 = GF.F16, GF.BF16, GF.F32
U = GF.U
Poisoned, Case = GF.Poisoned, GF.Case
_bits, _ulp, _ints, _round, _gemm, _dt_code, _lib = GF._bits, GF._ulp, GF._ints, GF._round, GF._gemm, GF._dt_code, GF._lib
_C_ACC = GF._C_ACC
_WORST = {}
TILES = (0, 64, 128, 256)  # the tile codes that accept a batch
DTYPES = pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
REGIMES = pytest.mark.parametrize("regime", ["exact", "real"])


def _bound(got, ref, acc_unit, epi_err, out_dt, what):
    """test_gemm_forms_gpu._bound under its bar, the worst ratio kept in this module's record"""
    GF._bound(got, ref, acc_unit, epi_err, out_dt, what)
    key = what.split(":")[0]
    if key in GF._WORST:
        _WORST[key] = max(_WORST.get(key, 0.0), GF._WORST.pop(key))


def _name(dt):
    return str(dt)[6:]


def _last_error():
    msg = _lib().lib().tcavt_last_error()
    return msg.decode() if msg else ""


def _refused(rc, C_buf, C_before, what):
    assert rc != 0, f"{what}: accepted"
    assert _last_error().startswith("gemm_bf16:"), f"{what}: last error {_last_error()!r}"
    assert torch.equal(_bits(C_buf), _bits(C_before)), f"{what}: a refused call wrote to C"


# ---------------------------------------------------------------------------------------------------------------------------
# host-rule mirrors

def _small_form(tile, M, N, batch):
    """launch_small (gemm_bf16.hip): the workgroup count includes the batch"""
    wgs = -(-M // 128) * -(-N // 128) * batch
    if tile == 64 or (tile == 0 and wgs <= 128):
        return "64"
    return "128p2" if wgs <= 256 else "128p1"


def _batched_form(tile, M, N, batch):
    """kernel form a batched generic call runs: tcavt_gemm_bf16's choice for tile 0 (256x256 tiles when they fill >= 75 % of whole
    waves of 256; the 4-wave forms take no batch), then dispatch_tile / launch_small"""
    if tile == 0:
        t256 = -(-M // 256) * -(-N // 256) * batch
        waves = -(-t256 // 256)
        if t256 >= 256 and t256 / (waves * 256) >= 0.75:
            return "256"
    return "256" if tile == 256 else _small_form(tile, M, N, batch)


def _drop_form(tile, M, N):
    """dropout_p > 0: launch_small<EPI_DROP> with the tile code if it is 64 or 128, else 0"""
    return _small_form(tile if tile in (64, 128) else 0, M, N, 1)


def test_form_coverage():
    """the docstring's tables: every small-launch form and the 8-wave form run batched, PIPE 1 with more than 256 workgroups
    counted over the batch; EPI_DROP runs as 64x64, 128x128 PIPE 2 and 128x128 PIPE 1"""
    for p in R.CALL_SITES + [R.BY_NAME["skinny_shaped"]]:
        assert [_batched_form(t, p.M, p.N, p.batch) for t in TILES] == ["64", "64", "128p2", "256"], p.name
    p = R.BY_NAME["pipe1_batch96"]
    assert -(-p.M // 128) * -(-p.N // 128) * p.batch > 256 >= -(-p.M // 128) * -(-p.N // 128)
    assert [_batched_form(t, p.M, p.N, p.batch) for t in TILES] == ["128p1", "64", "128p1", "256"]
    p = R.MAX_BATCH
    assert [_batched_form(t, p.M, p.N, p.batch) for t in TILES] == ["256", "64", "128p1", "256"]
    assert [_drop_form(t, 300, 208) for t in (64, 128, 0, 256)] == ["64", "128p2", "64", "64"]
    assert _drop_form(128, 2100, 2064) == "128p1" and -(-2100 // 128) * -(-2064 // 128) == 289 and 2100 % 128 and 2064 % 128


# ---------------------------------------------------------------------------------------------------------------------------
# batched form

class Batched:
    """Flat operand buffers of one pattern (NaN wherever no product reads), their float64 products and |A| |W|^T."""

    def __init__(self, p, dt, regime, seed, dev):
        self.p, self.dt, self.regime, self.dev = p, dt, regime, dev
        self.g = g = torch.Generator().manual_seed(seed)
        a_need, w_need, self.c_need = R.need(p)
        # (room for the W of every inner index, NaN where the group leaves it unread: a kernel that ignored batch_w_group would
        #  read NaN inside the buffer, not past its end)
        w_need = max(w_need, R.need(p.but(p.name, batch_w_group=1))[1])

        def data(n):
            return (_ints((n,), 4, g) if regime == "exact" else torch.randn(n, generator=g).double()).to(dev)

        nan = torch.tensor(float("nan"), dtype=dt, device=dev)
        if p.w_in_a >= 0:  # one buffer holds both operands
            n = max(a_need, p.w_in_a + w_need) + 64
            am, wm, _ = R.masks(p, n, n - p.w_in_a, 0, dev)
            am[p.w_in_a:] |= wm
            self.bufs = [torch.where(am, data(n).to(dt), nan)]
            self.A, self.W = self.bufs[0], self.bufs[0][p.w_in_a:]
        else:
            am, wm, _ = R.masks(p, a_need + 64, w_need + 64, 0, dev)
            self.A, self.W = torch.where(am, data(a_need + 64).to(dt), nan), torch.where(wm, data(w_need + 64).to(dt), nan)
            self.bufs = [self.A, self.W]
        self.before = [b.clone() for b in self.bufs]
        A64, W64 = self.A.double(), self.W.double()
        self.acc = R.batched_ref(A64, W64, p)
        self.abs = R.batched_ref(A64.abs(), W64.abs(), p)
        assert torch.isfinite(self.acc).all() and torch.isfinite(self.abs).all(), "a product reads an element outside the masks"
        self.c_len = max(p.c_off + self.c_need, p.c_total) + 64
        self.cmask = torch.zeros(self.c_len, dtype=torch.bool, device=dev)
        self.cmask[p.c_off:] = R.masks(p, 0, 0, self.c_len - p.c_off, dev)[2]

    def side(self, shape, den=4):
        """fp32 side input: dyadic small numbers in the exact regime, N(0, 1) otherwise"""
        if self.regime == "exact":
            return (torch.randint(-8 * den, 8 * den + 1, shape, generator=self.g).float() / den).to(self.dev)
        return torch.randn(shape, generator=self.g).to(self.dev)

    def new_c(self, out_dt):
        buf = torch.full((self.c_len,), float("nan"), dtype=out_dt, device=self.dev)
        return buf, buf.clone()

    def args(self, tile, C, out_dt, **kw):
        d = dict(self.p.fields(), A=self.A, W=self.W, C=C[self.p.c_off:], tile=tile, in_dtype=_dt_code(self.dt), out_dtype=_dt_code(out_dt))
        d.update(kw)
        return d

    def flat(self, vals):
        """per-product values [batch, M, N] laid out as the whole C buffer"""
        out = torch.full((self.c_len,), float("nan"), dtype=vals.dtype, device=self.dev)
        out[self.p.c_off:] = R.scatter_c(vals, self.p, self.c_len - self.p.c_off)
        return out

    def check_c(self, C, C_before, ref, acc_unit, epi_err, out_dt, what):
        """addressed elements: bit-equal to the rounded reference (exact) / within bound (real); every other element untouched"""
        m = self.cmask
        assert torch.equal(_bits(C)[~m], _bits(C_before)[~m]), f"{what}: write outside the products' regions"
        got, want = C[m], self.flat(ref)[m]
        assert torch.isfinite(got.double()).all(), f"{what}: {int((~torch.isfinite(got.double())).sum())} addressed elements not finite"
        if self.regime == "exact":
            w = _round(want, out_dt) if out_dt != F32 else want.float()
            bad = _bits(got) != _bits(w)
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ, first at flat index {m.nonzero()[bad.nonzero()[0]].item()}"
        else:
            _bound(got, want, self.flat(acc_unit)[m], self.flat(epi_err)[m], out_dt, what)

    def check_inputs(self, what):
        for b, k in zip(self.bufs, self.before):
            assert torch.equal(_bits(b), _bits(k)), f"{what}: an operand buffer was modified"


def _run_batched(bt, what0, epilogue=0, bias=None, brow=None, res=None, acc_scale=1.0, tiles=TILES):
    """the pattern under every tile code and both output types, each against float64; the tile codes bit-identical"""
    capi = _lib()
    p = bt.p
    ref = bt.acc * acc_scale
    mag = 0
    if bias is not None:
        ref = ref + bias.double()[None, None, :]
        mag = mag + bias.double().abs()[None, None, :]
    if brow is not None:
        ref = ref + brow.double()[None, :, None]
        mag = mag + brow.double().abs()[None, :, None]
    if epilogue & capi.EPI_RELU:
        ref = ref.clamp_min(0)
    mag = mag + ref.abs()
    if res is not None:  # one [M, N] residual, shared by all products
        ref = ref + res.double()[None]
        mag = mag + res.double().abs()[None]
    kw = dict(epilogue=epilogue, acc_scale=acc_scale)
    if bias is not None or brow is not None:
        kw.update(bias=bias if bias is not None else brow)
    if res is not None:
        kw.update(residual=res, ldr=p.N)
    side = [t for t in (bias, brow, res) if t is not None]
    keep = [t.clone() for t in side]
    for out_dt in (F32, bt.dt):
        outs = {}
        for tile in tiles:
            what = f"batched {what0} {_name(bt.dt)}: ->{_name(out_dt)} {bt.regime}, tile {tile} ({_batched_form(tile, p.M, p.N, p.batch)})"
            C, C_before = bt.new_c(out_dt)
            capi.check(_gemm(**bt.args(tile, C, out_dt, **kw)), what)
            bt.check_c(C, C_before, ref, acc_scale * U * bt.abs, 4 * U * mag, out_dt, what)
            bt.check_inputs(what)
            outs[tile] = C
        for tile in tiles:
            assert torch.equal(_bits(outs[tile]), _bits(outs[tiles[0]])), f"{what0} {_name(out_dt)}: tile {tile} differs from tile {tiles[0]}"
    for t, k in zip(side, keep):
        assert torch.equal(_bits(t), _bits(k)), f"{what0}: a side input was modified"


@REGIMES
@DTYPES
@pytest.mark.parametrize("p", R.PATTERNS, ids=lambda p: p.name)
def test_batched(gpu, p, dt, regime):
    """every call-site pattern (acc_scale / BIAS_ROW as the call site passes them), PIPE 1 with the workgroups counted over the
    batch, and the skinny-shaped batch"""
    capi = _lib()
    bt = Batched(p, dt, regime, seed=p.M * 7 + p.K + p.batch + len(p.name), dev=gpu["device"])
    brow = bt.side((p.M,)) if p.bias_row else None
    _run_batched(bt, p.name, epilogue=capi.EPI_BIAS_ROW if p.bias_row else 0, brow=brow, acc_scale=p.acc_scale)


@REGIMES
@DTYPES
def test_batched_shared_side_inputs(gpu, dt, regime):
    """bias and residual are shared by all products (include/tcavt.h): xattn_scores with BIAS | RELU | RESIDUAL and ONE [M, N]
    residual, which the reference adds to every product"""
    capi = _lib()
    p = R.BY_NAME["xattn_scores"]
    bt = Batched(p, dt, regime, seed=77, dev=gpu["device"])
    _run_batched(bt, "xattn_scores_bias_relu_res", epilogue=capi.EPI_BIAS | capi.EPI_RELU | capi.EPI_RESIDUAL, bias=bt.side((p.N,)),
                 res=bt.side((p.M, p.N), den=8), acc_scale=p.acc_scale)


@DTYPES
@pytest.mark.parametrize("name", ["gqa_scores_wg0", "gqa_dq_wg0"])
def test_w_group_zero_is_one(gpu, name, dt):
    """batch_w_group = 0 and = 1 are the same call, bit for bit"""
    capi = _lib()
    p = R.BY_NAME[name]
    bt = Batched(p, dt, "real", seed=5, dev=gpu["device"])
    for out_dt in (F32, dt):
        for tile in TILES:
            outs = []
            for wg in (0, 1):
                C, _ = bt.new_c(out_dt)
                capi.check(_gemm(**bt.args(tile, C, out_dt, acc_scale=p.acc_scale, batch_w_group=wg)), f"{name} w_group {wg}")
                outs.append(C)
            assert torch.equal(_bits(outs[0]), _bits(outs[1])), (name, tile, out_dt)
            assert torch.isfinite(outs[0][bt.cmask].double()).all()


@REGIMES
@DTYPES
def test_max_batch(gpu, dt, regime):
    """batch = 65535 (the limit of blockIdx.y): all products read one operand pair and write contiguous 16 x 16 blocks, every one
    of them compared with the single float64 product"""
    capi = _lib()
    dev = gpu["device"]
    p = R.MAX_BATCH
    g = torch.Generator().manual_seed(65535)
    vals = [(_ints((r * p.K,), 4, g) if regime == "exact" else torch.randn(r * p.K, generator=g).double()) for r in (p.M, p.N)]
    A, W = (torch.cat([v.to(dt), torch.full((64,), float("nan"), dtype=dt)]).to(dev) for v in vals)
    keep = [A.clone(), W.clone()]
    a64, w64 = A[: p.M * p.K].double().view(p.M, p.K), W[: p.N * p.K].double().view(p.N, p.K)
    ref, unit = a64 @ w64.T, U * (a64.abs() @ w64.abs().T)
    n = p.batch * p.M * p.N
    for out_dt in (F32, dt):
        outs = {}
        for tile in TILES:
            what = f"batched max_batch {_name(dt)}: ->{_name(out_dt)} {regime}, tile {tile} ({_batched_form(tile, p.M, p.N, p.batch)})"
            C = torch.full((n + 64,), float("nan"), dtype=out_dt, device=dev)
            capi.check(_gemm(**dict(p.fields(), A=A, W=W, C=C, tile=tile, in_dtype=_dt_code(dt), out_dtype=_dt_code(out_dt))), what)
            assert torch.isnan(C[n:]).all(), f"{what}: write past the last product"
            got = C[:n].view(p.batch, p.M, p.N)
            if regime == "exact":
                want = _round(ref, out_dt) if out_dt != F32 else ref.float()
                bad = (_bits(got) != _bits(want)[None]).flatten(1).any(1)
                assert not bool(bad.any()), f"{what}: {int(bad.sum())} products differ, first {int(bad.nonzero()[0])}"
            else:
                _bound(got, ref[None].expand_as(got), unit[None].expand_as(got), 4 * U * ref.abs()[None].expand_as(got), out_dt, what)
            outs[tile] = C
        for tile in TILES:
            assert torch.equal(_bits(outs[tile]), _bits(outs[0])), (tile, out_dt)
    assert torch.equal(_bits(A), _bits(keep[0])) and torch.equal(_bits(W), _bits(keep[1]))


def test_batched_refusals(gpu):
    """what a batched call may not be: each returns nonzero with a gemm_bf16 message and leaves C alone; the same call with
    batch = 1 (or the one bad field put right) is accepted, so the batch is what was refused"""
    capi = _lib()
    dev = gpu["device"]
    p = R.BY_NAME["xattn_scores"]
    bt = Batched(p, F16, "real", seed=3, dev=dev)
    M, N = p.M, p.N
    cos, sin = torch.ones(M, 32, device=dev), torch.zeros(M, 32, device=dev)
    h16 = torch.zeros(bt.c_len, dtype=F16, device=dev)
    part = torch.zeros(M * (N // 64) * p.batch, device=dev)
    rope = dict(epilogue=capi.EPI_ROPE, rope_cos=cos, rope_sin=sin, rope_L=M, rope_cols=N)
    norm = dict(epilogue=capi.EPI_NORM_OUT, norm_h16=h16, norm_part=part)
    drop = dict(dropout_p=0.25, dropout_seed=1, dropout_site=1)
    cases = [("SILU_MUL", dict(epilogue=capi.EPI_SILU_MUL), True), ("ROPE", rope, True), ("NORM_OUT", norm, True), ("dropout", drop, True),
             ("w_layout", dict(w_layout=capi.W_FRAG16), False), ("act_layout", dict(act_layout=1), False),
             ("batch % batch_inner", dict(batch_inner=4), False), ("sAo % 8", dict(sAo=p.sAo + 4), False),
             ("sWi % 8", dict(sWi=p.sWi + 4), False), ("sCo % 4", dict(sCo=p.sCo + 2), False), ("batch 65536", dict(batch=65536), False)]
    C, C_before = bt.new_c(F32)
    capi.check(_gemm(**bt.args(0, C, F32)), "the call the refusals are variations of")
    for what, kw, twin in cases:
        C, C_before = bt.new_c(F32)
        _refused(_gemm(**bt.args(0, C, F32, **kw)), C, C_before, f"batch with {what}")
        if twin:
            capi.check(_gemm(**bt.args(0, C, F32, **dict(kw, batch=1))), f"{what} without a batch")
    # the 4-wave tile codes: whole 256-row / 256- and 192-column tiles, so that the batch is all that is wrong
    q = R._contiguous("w4", 512, 768, 256, 2, 1, "")
    b4 = Batched(q, F16, "real", seed=4, dev=dev)
    for tile in (257, 271, 272):
        C, C_before = b4.new_c(F16)
        _refused(_gemm(**b4.args(tile, C, F16)), C, C_before, f"batch with tile {tile}")
        capi.check(_gemm(**b4.args(tile, C, F16, batch=1)), f"tile {tile} without a batch")
    bt.check_inputs("refusals")
    b4.check_inputs("refusals")


def test_gemm_batched_extent_guard(gpu):
    """ops.gemm_batched asks each buffer for exactly what the products address, w_group included: with a, w and out `need`
    elements long the call runs; one element shorter it raises, names the tensor and launches nothing"""
    from tcavt_amd import ops

    capi = _lib()
    dev = gpu["device"]
    for name in ("gqa_dq", "gqa_dq_wg0"):
        p = R.BY_NAME[name]
        need = dict(zip(("a", "w", "out"), R.need(p)))
        g = torch.Generator().manual_seed(9)
        kw = dict(M=p.M, N=p.N, K=p.K, lda=p.lda, ldw=p.ldw, ldc=p.ldc, batch=p.batch, inner=p.batch_inner, sA=p.sA, sW=p.sW, sC=p.sC,
                  tile=64, w_group=p.batch_w_group)

        def tensors(short=None):
            t = {k: torch.randn(n - (k == short), generator=g).to(F16).to(dev) for k, n in need.items() if k != "out"}
            t["out"] = torch.full((need["out"] - (short == "out"),), float("nan"), device=dev)
            return t

        t = tensors()
        ops.gemm_batched(t["a"], t["w"], t["out"], **kw)
        torch.cuda.synchronize()
        cm = R.masks(p, 0, 0, need["out"], dev)[2]
        ref = R.scatter_c(R.batched_ref(t["a"].double(), t["w"].double(), p), p, need["out"])
        unit = R.scatter_c(R.batched_ref(t["a"].double().abs(), t["w"].double().abs(), p), p, need["out"])
        _bound(t["out"][cm], ref[cm], U * unit[cm], 4 * U * ref[cm].abs(), F32, f"batched extent_guard: {name}")
        assert torch.isnan(t["out"][~cm]).all()
        for short in ("a", "w", "out"):
            t = tensors(short)
            with pytest.raises(capi.TcavtError, match=rf"gemm_batched\.{short}:"):
                ops.gemm_batched(t["a"], t["w"], t["out"], **kw)
            torch.cuda.synchronize()
            assert torch.isnan(t["out"]).all(), f"{name}: launched with {short} one element short"
    # a group of 2 needs fewer W operands than no group: what suffices for w_group = 2 is refused for w_group = 1
    p, p1 = R.BY_NAME["gqa_dq"], R.BY_NAME["gqa_dq_wg0"]
    assert R.need(p)[1] < R.need(p1)[1]
    t = tensors()
    w2 = torch.randn(R.need(p)[1], generator=g).to(F16).to(dev)
    t["out"].fill_(float("nan"))
    with pytest.raises(capi.TcavtError, match=r"gemm_batched\.w:"):
        ops.gemm_batched(t["a"], w2, t["out"], **dict(kw, w_group=1))
    torch.cuda.synchronize()
    assert torch.isnan(t["out"]).all()
    ops.gemm_batched(t["a"], w2, t["out"], **dict(kw, w_group=2))
    torch.cuda.synchronize()
    assert torch.isfinite(t["out"][R.masks(p, 0, 0, t["out"].numel(), dev)[2]]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# dropout epilogue

SEED, SITE = 0x1234567890ABCDEF, 7  # a seed above 2^32: both key words matter
P_EDGE = 2.0 ** -16  # keep threshold 1: only a draw of 0 drops


@functools.lru_cache(maxsize=None)
def _keep_cpu(n, p, seed, site):
    from oracle import philox

    return torch.from_numpy(philox.keep_mask(n, p, seed, site))


def _keep(M, N, p, site, dev):
    """keep mask of the [M, N] output: flat index m * N + n, whatever ldc is"""
    return _keep_cpu(M * N, p, SEED, site).view(M, N).to(dev)


DROP_SHAPES = [((64, 128, 0, 256), 300, 208, 256), ((128,), 2100, 2064, 128)]


@pytest.mark.parametrize("mode", ["exact", "real", "edge"])
@DTYPES
@pytest.mark.parametrize("shape", DROP_SHAPES, ids=lambda s: GF._id(s[1:]))
def test_dropout(gpu, shape, dt, mode):
    """EPI_DROP on every form that has it, per element: exact (p = 0.5, the scale is 2: bit for bit), real (p = 0.1) and the
    threshold edge (p = 2^-16, real operands).  Tile codes at one shape give bit-identical results; tile 256 is served by the
    small kernels and equals tile 0"""
    from tcavt_amd import ops

    tiles, M, N, K = shape
    dev = gpu["device"]
    capi = _lib()
    ops.set_dropout_epoch(None)  # masks are a function of (seed, site, element) alone
    regime = "exact" if mode == "exact" else "real"
    p = {"exact": 0.5, "real": 0.1, "edge": P_EDGE}[mode]
    s64 = 1.0 / (1.0 - float(torch.tensor(p, dtype=F32)))
    keep = _keep(M, N, p, SITE, dev)
    assert 0 < int((~keep).sum()) < M * N
    cs = Case(M, N, K, dt, regime, seed=M + N + K + 5, dev=dev)
    bias, res = cs.side((N,)), cs.side((M, N), scale=4.0, den=8)
    sides = [bias.clone(), res.clone()]
    BR = capi.EPI_BIAS | capi.EPI_RELU
    variants = [("plain", 0), ("bias_relu", BR), ("bias_relu_res", BR | capi.EPI_RESIDUAL), ("res_inplace", BR | capi.EPI_RESIDUAL)]
    for out_dt in (F32, dt):
        for name, epi in variants:
            if name == "res_inplace" and out_dt != F32:
                continue
            pre = cs.acc
            if epi & capi.EPI_BIAS:
                pre = (pre + bias.double()).clamp_min(0)
            scaled = pre * keep * s64
            ref = scaled + res.double() if epi & capi.EPI_RESIDUAL else scaled
            mag = scaled.abs() + keep * s64 * (bias.double().abs() if epi & capi.EPI_BIAS else 0) + (res.double().abs() if epi & capi.EPI_RESIDUAL else 0)
            # the generic bound on the kept value, scaled, + 2 ulp_fp32 of the scaled value: the fp32 scale 1 / (1 - p) and the multiply
            acc_unit, epi_err = keep * s64 * U * cs.abs, 4 * U * mag + 2 * _ulp(scaled, F32)
            outs = {}
            for tile in tiles:
                what = f"drop {_drop_form(tile, M, N)} {_name(dt)} {mode}: {name} ->{_name(out_dt)}, tile {tile}, {M}x{N}x{K}"
                C = Poisoned(M, N, out_dt, dev, fill=res if name == "res_inplace" else None)
                kw = dict(bias=bias) if epi & capi.EPI_BIAS else {}
                if epi & capi.EPI_RESIDUAL:
                    kw.update(residual=C.buf, ldr=C.ld) if name == "res_inplace" else kw.update(residual=res, ldr=N)
                rc = _gemm(**cs.args(tile, C=C.buf, ldc=C.ld, out_dtype=_dt_code(out_dt), epilogue=epi, dropout_p=p, dropout_seed=SEED,
                                     dropout_site=SITE, **kw))
                capi.check(rc, what)
                got = C.region
                if regime == "exact":
                    want = _round(ref, out_dt) if out_dt != F32 else ref.float()
                    bad = _bits(got) != _bits(want)
                    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ, first {bad.nonzero()[0].tolist()}"
                else:
                    _bound(got, ref, acc_unit, epi_err, out_dt, what)
                # dropped elements: exactly the residual, or zero (+0 after a ReLU; 0 * x keeps x's sign without one, as in the reference)
                if epi or regime == "exact":
                    dropped = res.to(out_dt) if epi & capi.EPI_RESIDUAL else (torch.zeros(M, N, dtype=out_dt, device=dev) if epi else (0.0 * cs.acc).to(out_dt))
                    assert torch.equal(_bits(got)[~keep], _bits(dropped)[~keep]), f"{what}: a dropped element is not exactly residual / 0"
                else:  # (the sign of 0 * x is that of the fp32 accumulator, which float64 does not pin down next to zero)
                    assert bool((got[~keep] == 0).all()), f"{what}: a dropped element is not 0"
                C.check(what)
                cs.check_inputs()
                outs[tile] = got.clone()
            for tile in tiles:
                assert torch.equal(_bits(outs[tile]), _bits(outs[tiles[0]])), f"drop {name} {_name(out_dt)} {mode}: tile {tile} differs from tile {tiles[0]}"
            if name == "bias_relu_res":  # another site: another mask
                C = Poisoned(M, N, out_dt, dev)
                capi.check(_gemm(**cs.args(tiles[0], C=C.buf, ldc=C.ld, out_dtype=_dt_code(out_dt), epilogue=epi, dropout_p=p,
                                           dropout_seed=SEED, dropout_site=SITE + 1, **kw)), "site + 1")
                k1 = _keep(M, N, p, SITE + 1, dev)
                assert not torch.equal(k1, keep)
                differs = _bits(C.region) != _bits(outs[tiles[0]])
                assert bool(differs.any()) and not bool(differs[k1 == keep].any()), "site + 1: the output differs exactly where the masks do"
    for t, k in zip((bias, res), sides):
        assert torch.equal(_bits(t), _bits(k))


def test_dropout_refusals(gpu):
    capi = _lib()
    dev = gpu["device"]
    M, N, K = 300, 256, 128
    cs = Case(M, N, K, F16, "real", seed=8, dev=dev)
    cos, sin = torch.ones(M, 32, device=dev), torch.zeros(M, 32, device=dev)
    h16, part = torch.zeros(M + 2, N + 16, dtype=F16, device=dev), torch.zeros(M * (N // 64), device=dev)
    drop = dict(dropout_p=0.1, dropout_seed=SEED, dropout_site=SITE)
    cases = [("p = 1", dict(drop, dropout_p=1.0), None), ("p < 0", dict(drop, dropout_p=-0.1), None),
             ("SILU_MUL", dict(drop, epilogue=capi.EPI_SILU_MUL), F16),
             ("ROPE", dict(drop, epilogue=capi.EPI_ROPE, rope_cos=cos, rope_sin=sin, rope_L=M, rope_cols=N), F16),
             ("NORM_OUT", dict(drop, epilogue=capi.EPI_NORM_OUT, norm_h16=h16, norm_part=part), F32)]
    for what, kw, twin_dt in cases:
        out_dt = twin_dt or F32
        C = Poisoned(M, N, out_dt, dev)
        _refused(_gemm(**cs.args(128, C=C.buf, ldc=C.ld, out_dtype=_dt_code(out_dt), **kw)), C.buf, C.before, f"dropout with {what}")
        if twin_dt is not None:  # the same call without dropout is accepted
            capi.check(_gemm(**cs.args(128, C=C.buf, ldc=C.ld, out_dtype=_dt_code(out_dt), **dict(kw, dropout_p=0.0))), f"{what} without dropout")
    cs.check_inputs()


def test_report_worst_ratio(gpu):
    """(runs last in file order) prints the worst accumulator ratio c measured per case in this session and holds it to the bar"""
    for k in sorted(_WORST):
        print(f"worst c  {k:50s} {_WORST[k]:.3f}")
    assert all(v <= _C_ACC for v in _WORST.values())
