"""tcavt_gemm_f32 and tcavt_gemm_f32_strided (csrc/small.hip) against float64, per element, on every path of launch_gemm_f32:
unsplit, the no-workspace 2-split through atomics into the zeroed C, split-K through workspace slices added in order.

Every case calls the C entry point (capi.lib().tcavt_gemm_f32*) and checks every element against ONE float64 evaluation in torch on
the CPU, from the same fp32 values; nothing in a reference comes from a project kernel.  Operands carry NaN columns behind K (or
behind the rows, when stored row-fast) and NaN rows behind them; C lies between NaN guard rows, with ldc == N and with ldc = N + 5
(five NaN guard columns); bias and a separate residual have NaN behind them: every in-range element comes back finite and inside
its bound, every guard keeps its bits, every input stays bit-unchanged, a second launch gives the same bits.

Regimes:
- integer: operands, bias, residual, the ACCUM start in [-3, 3]: every partial sum is an integer below 2^24 (asserted), so the
  result is exact in any order and every form -- split-K through atomics and through the workspace included -- must equal the
  float64 value bit for bit.
- realistic: N(0, 1), per-element bound (bar 1.0)
      1.01 * [chain E S + nops E U] + ulp_fp32(ref),   S = sum_k |a| |w|,   U = S + |C0| + |bias| + |residual|
  chain = the k-chain of one workgroup (K, or the longest chunk of a split: the MFMA accumulates like an fmaf chain, one rounding
  per k), nops = the additions behind it: one per further split, one per ACCUM / BIAS / RESIDUAL.  ReLU does not widen an error;
  dropout (p = 0.5, 1 / (1 - p) = 2 exact) doubles what it keeps.

tcavt_gemm_f32 (M, N, K): (1,1,1) smallest; (63,65,15) (64,64,16) (65,63,17) tile and K-step edges; (130,70,33) several tiles;
(5,3,511) just below the split threshold; (5,3,512) two chunks of 256; (70,130,520) chunks of 272 and 248; (64,64,1000) chunks of
512 and 488.  Flags: none, BIAS, BIAS|RELU, BIAS|RESIDUAL, BIAS|RELU|RESIDUAL, RESIDUAL aliasing C (in place) -- each with both
ldc, at every shape, so the cases where the host rule must NOT split (RELU, ldc > N, residual aliasing C) are all called at the
three K >= 512 shapes; test_cases_cover_the_host_rules lists which cases split.
Dropout: p = 0.5 at (70,33,50) and (65,63,17), BIAS|RELU|RESIDUAL, ldc > N: bias -> ReLU -> oracle.philox.keep_mask at m * N + n
-> residual.  NaN: one NaN in a row of A with RELU makes that output row NaN (relu_nan; the non-finite-loss gate relies on it),
every other row stays finite and inside its bound.

tcavt_gemm_f32_strided: all four operand orientations (A k-fast / row-fast x W k-fast / row-fast) at (65,63,17), (70,130,520)
with an 8-slice NaN workspace (2 slices written, the rest still NaN), (64,64,1000) (3 slices), and (1,63,17), (65,63,1) with
unpadded operands, where the two strides of an operand tie.  Flags: none, ACCUM onto a non-zero C, BIAS|RESIDUAL, RELU (unsplit).
Without a workspace at the two K >= 512 shapes: ldc == N (2 splits through atomics), ldc > N and the residual aliasing C (unsplit).

Refusals pass only arguments that the host code rejects before any launch (NULL pointers, M = 0, ACCUM with RELU, a flag the entry
does not take, BIAS without bias, dropout_p = 1).

MEASURED on an MI355X: the worst fraction of the bound per path stands beside the constants below;
profiles/fp32_train_tail_bounds.txt has every line and the mutants; test_report_worst_ratio prints the session's (pytest -s).
"""
import pytest
import torch

from test_attention_bwd_gpu import _first_bad, _last_error
from test_gemm_forms_gpu import Poisoned, _bits, _ulp
from test_head_forward_kernels_gpu import _dev
from test_llm_backward_kernels_gpu import SEED, Guarded, _gen, _L, _ok, _st

pytestmark = pytest.mark.gpu

F32 = torch.float32
_E = 2.0 ** -24   # unit roundoff of fp32
BIAS, RELU, RES, ACCUM = 1, 2, 4, 64      # TCAVT_EPI_* (asserted against capi in test_cases_cover_the_host_rules)
# MEASURED on an MI355X: worst fraction of the whole bound (bar 1.0) over the realistic cases, per path
#   tcavt_gemm_f32          unsplit 0.267   2 splits through atomics 0.008
#   tcavt_gemm_f32_strided  unsplit 0.502 (K = 1: the one rounding of the product)   atomics 0.009   workspace slices 0.009
# (a split's chain term, 272 .. 512 E S, is a worst case that random data stays far below; there the integer regime is the sharp check)
# Mutants (profiles/fp32_train_tail_bounds.txt): ldc == N dropped from the no-workspace split rule, residual != C dropped from it,
# ReLU before bias, dropout after the residual: each fails here; `gk < K` for `gk < ke` in the fetch guard is equivalent as long as
# the host rounds k_chunk up to the K-step (with k_chunk left unrounded as well it fails the three split tests at both K > 512 shapes).
_WORST = {}

REGIMES = ["integer", "realistic"]
F32_SHAPES = [(1, 1, 1), (63, 65, 15), (64, 64, 16), (65, 63, 17), (130, 70, 33), (5, 3, 511), (5, 3, 512), (70, 130, 520), (64, 64, 1000)]
FLAGSETS = [("none", 0, False), ("bias", BIAS, False), ("bias|relu", BIAS | RELU, False), ("bias|res", BIAS | RES, False),
            ("bias|relu|res", BIAS | RELU | RES, False), ("res in place", RES, True)]       # (name, flags, residual aliases C)
LDC_PADS = [0, 5]
DROP_SHAPES = [(70, 33, 50), (65, 63, 17)]
NAN_SHAPES = [(65, 63, 17), (70, 130, 520)]
ORIENTS = [("k", "k"), ("k", "r"), ("r", "k"), ("r", "r")]                                 # (A, W): k-fast or row-fast
STRIDED_SHAPES = [(65, 63, 17), (70, 130, 520), (64, 64, 1000)]
TIE_SHAPES = [(1, 63, 17), (65, 63, 1)]
STRIDED_FLAGS = [("none", 0), ("accum", ACCUM), ("bias|res", BIAS | RES), ("relu", RELU)]
WS_SLICES = 8
NO_WS = [("ldc == N", 0, 0, False), ("ldc > N", 0, 5, False), ("res in place", RES, 0, True)]   # (name, flags, ldc - N, alias)


def _plan(max_splits, M, N, K, flags, ldc, alias, ws_slices=0, dropout=0.0):
    """launch_gemm_f32 mirrored: (path, splits, k_chunk)"""
    tiles = -(-N // 64) * -(-M // 64)
    splits = 1
    if tiles < 128 and K >= 512 and not flags & RELU and dropout == 0.0:
        cap = 0
        if ws_slices:
            cap = min(max_splits, ws_slices)        # ws_elems / (M * N) with ws_elems = ws_slices * M * N
        elif not flags & ACCUM and not alias and ldc == N:
            cap = min(max_splits, 2)
        splits = min(K // 256, cap)
        while splits > 1 and tiles * splits > 512:
            splits >>= 1
        splits = max(splits, 1)
    if splits == 1:
        return "unsplit", 1, K
    k_chunk = -(-(-(-K // splits)) // 16) * 16
    splits = -(-K // k_chunk)
    return ("ws" if ws_slices else "atomic"), splits, k_chunk


def _chunks(K, splits, k_chunk):
    return [min(K, (z + 1) * k_chunk) - z * k_chunk for z in range(splits)]


def _strides(orient, rows, K, pad):
    """(buffer rows, buffer columns, ld, row stride, k stride) of an operand X[row][k] stored k-fast ([rows][K]) or row-fast ([K][rows])"""
    r, c = (rows, K) if orient == "k" else (K, rows)
    ld = c + (3 if pad else 0)
    return (r, c, ld, ld, 1) if orient == "k" else (r, c, ld, 1, ld)


def test_cases_cover_the_host_rules():
    """from the case lists alone (launch_gemm_f32 mirrored): every path and edge is reached; which cases split"""
    from tcavt_amd import capi

    assert (capi.EPI_BIAS, capi.EPI_RELU, capi.EPI_RESIDUAL, capi.EPI_ACCUM) == (BIAS, RELU, RES, ACCUM)
    # tcavt_gemm_f32: max_splits = 2, no workspace
    split = {}
    for M, N, K in F32_SHAPES:
        for name, flags, alias in FLAGSETS:
            for pad in LDC_PADS:
                path, s, kc = _plan(2, M, N, K, flags, N + pad, alias)
                assert path in ("unsplit", "atomic")
                if path == "atomic":
                    split[(M, N, K, name, pad)] = _chunks(K, s, kc)
                # the host rule: K >= 512, no ReLU, ldc == N, the residual not aliasing C
                assert (path == "atomic") == (K >= 512 and not flags & RELU and pad == 0 and not alias)
    assert {k[:3]: v for k, v in split.items()} == {(5, 3, 512): [256, 256], (70, 130, 520): [272, 248], (64, 64, 1000): [512, 488]}
    assert {k[3] for k in split} == {"none", "bias", "bias|res"} and {k[4] for k in split} == {0}
    assert any(c[-1] % 16 for c in split.values())                                     # a split whose tail is no multiple of 16
    big = [s for s in F32_SHAPES if s[2] >= 512]
    assert len(big) == 3 and (5, 3, 511) in F32_SHAPES                                 # just below the threshold
    reasons = {("relu " if f & RELU else "") + ("ldc " if pad else "") + ("alias" if al else "") for _, f, al in FLAGSETS for pad in LDC_PADS}
    assert {"relu ", "ldc ", "alias"} <= reasons                                      # every reason not to split is called alone, at each of them
    dims = {(M % 64, N % 64, K % 16) for M, N, K in F32_SHAPES}
    assert {(63, 1, 15), (0, 0, 0), (1, 63, 1)} <= dims and any(M > 128 for M, _, _ in F32_SHAPES) and any(N > 128 for _, N, _ in F32_SHAPES)
    # dropout and ReLU never split
    assert all(_plan(2, M, N, K, BIAS | RELU | RES, N + 5, False, dropout=0.5)[0] == "unsplit" for M, N, K in DROP_SHAPES)
    # tcavt_gemm_f32_strided: max_splits = 8
    got = {}
    for M, N, K in STRIDED_SHAPES + TIE_SHAPES:
        for name, flags in STRIDED_FLAGS:
            got[(M, N, K, name)] = _plan(8, M, N, K, flags, N, False, ws_slices=WS_SLICES)
    assert all(v[0] == "unsplit" for k, v in got.items() if k[2] < 512 or k[3] == "relu")
    for name in ("none", "accum", "bias|res"):
        assert got[(70, 130, 520, name)] == ("ws", 2, 272) and got[(64, 64, 1000, name)] == ("ws", 3, 336)
    assert _chunks(1000, 3, 336) == [336, 336, 328]
    for M, N, K in STRIDED_SHAPES[1:]:
        assert [_plan(8, M, N, K, f, N + pad, al)[0] for _, f, pad, al in NO_WS] == ["atomic", "unsplit", "unsplit"]
    assert len(set(ORIENTS)) == 4
    # the kernel reads an operand along k when csX <= rsX: both branches, and the tie, for A and for W
    for dim in (0, 1):                                                                 # A has M rows, W has N
        cmp = set()
        for s in STRIDED_SHAPES + TIE_SHAPES + [(1, 1, 1)]:
            for o in "kr":
                _, _, _, rs, cs = _strides(o, s[dim], s[2], pad=s in STRIDED_SHAPES)
                cmp.add((cs > rs) - (cs < rs))
        assert cmp == {-1, 0, 1}
    assert any(_strides("r", M, K, False)[3:] == (1, 1) for M, _, K in TIE_SHAPES) and any(_strides("k", M, K, False)[3:] == (1, 1) for M, _, K in TIE_SHAPES)


# ---------------------------------------------------------------------------------------------------------------------------
# data, launch, reference and bound

def _data(shape, regime, g_):
    if regime == "integer":
        return torch.randint(-3, 4, shape, generator=g_).double()
    return torch.randn(shape, generator=g_).double()


class _Operand:
    """X[row][k] in a NaN-padded buffer, k-fast or row-fast; .vals is the float64 [rows, K] view of what the kernel reads"""

    def __init__(self, vals, orient, dev, pad=True):
        rows, K = vals.shape
        r, c, ld, self.rs, self.cs = _strides(orient, rows, K, pad)
        self.p = Poisoned(r, c, F32, dev, ld=ld, extra_rows=3, fill=vals if orient == "k" else vals.T)
        v = self.p.region.double().cpu()
        self.vals = v if orient == "k" else v.T
        self.ptr = self.p.buf.data_ptr()

    def unchanged(self, what):
        assert torch.equal(_bits(self.p.buf), _bits(self.p.before)), f"{what}: operand modified"


def _run(entry, dev, regime, M, N, K, flags, ldc_pad, alias, seed, oa="k", ow="k", pad=True, ws_slices=0, dropout=0.0, site=0, nan_row=None):
    """one case: two launches into fresh outputs (guards, inputs, reproducibility), the float64 reference, the judgement"""
    g_ = _gen(seed)
    a, w = _data((M, K), regime, g_), _data((N, K), regime, g_)
    if nan_row is not None:
        a[nan_row, K // 2] = float("nan")
    A, W = _Operand(a, oa, dev, pad), _Operand(w, ow, dev, pad)
    bias = _dev(_data((1, N), regime, g_), dev) if flags & BIAS else None
    rvals = _data((M, N), regime, g_).float() if flags & RES else None
    c0 = _data((M, N), regime, g_).float() if flags & ACCUM else None
    res = Poisoned(M, N, F32, dev, ld=N + 7, extra_rows=3, fill=rvals) if flags & RES and not alias else None
    ldc = N + ldc_pad
    strided = entry == "tcavt_gemm_f32_strided"
    path, splits, k_chunk = _plan(8 if strided else 2, M, N, K, flags, ldc, alias, ws_slices, dropout)
    what = (f"{entry} {regime} {(M, N, K)} flags={flags} ldc=N+{ldc_pad}{' in place' if alias else ''} A:{oa} W:{ow}"
            f"{f' ws={ws_slices}' if ws_slices else ''}{f' p={dropout}' if dropout else ''} [{path} x{splits}]")
    runs = []
    for tag in ("", " again"):
        C = Guarded(M, N, F32, dev, ld=ldc, fill=rvals if alias else c0, before=4, after=4)
        ws = torch.full((ws_slices * M * N + 64,), float("nan"), device=dev) if ws_slices else None
        rp, ldr = (C.ptr, ldc) if alias else (res.buf.data_ptr(), res.ld) if res is not None else (None, 0)
        bp = bias.buf.data_ptr() if bias is not None else None
        if strided:
            rc = _L().tcavt_gemm_f32_strided(A.ptr, A.rs, A.cs, W.ptr, W.rs, W.cs, bp, rp, ldr, C.ptr, ldc, M, N, K, flags,
                                             ws.data_ptr() if ws is not None else None, ws_slices * M * N, _st())
        else:
            rc = _L().tcavt_gemm_f32(A.ptr, A.rs, W.ptr, W.rs, bp, rp, ldr, C.ptr, ldc, M, N, K, flags, dropout, SEED, site, _st())
        _ok(rc, what + tag)
        C.check(what + tag)
        A.unchanged(what + tag + " A")
        W.unchanged(what + tag + " W")
        for x, nm in ((bias, "bias"), (res, "residual")):
            assert x is None or torch.equal(_bits(x.buf), _bits(x.before)), f"{what}{tag}: {nm} modified"
        if ws is not None:
            used = splits * M * N if path == "ws" else 0
            assert bool(torch.isfinite(ws[:used]).all()) or nan_row is not None, what + tag + ": a workspace slice in use was not written"
            assert bool(torch.isnan(ws[used:]).all()), what + tag + f": the workspace was written beyond its {used // (M * N)} slices in use"
        runs.append(C)
    assert torch.equal(_bits(runs[0].buf), _bits(runs[1].buf)), what + ": not reproducible"
    # the reference: bias -> ReLU -> dropout -> residual, ACCUM before the bias
    a64, w64 = A.vals, W.vals
    if nan_row is not None:
        a64 = torch.nan_to_num(a64, nan=0.0)
    val, S = a64 @ w64.T, a64.abs() @ w64.abs().T
    U, nops = S.clone(), splits - 1
    chain = max(_chunks(K, splits, k_chunk))
    if flags & ACCUM:
        val, U, nops = val + c0.double(), U + c0.double().abs(), nops + 1
    if flags & BIAS:
        b64 = bias.region.double().cpu()
        val, U, nops = val + b64, U + b64.abs(), nops + 1
    if flags & RELU:
        val = val.clamp_min(0.0)
    err = chain * _E * S + nops * _E * U
    if dropout:
        from oracle.philox import keep_mask

        assert dropout == 0.5
        keep = torch.from_numpy(keep_mask(M * N, dropout, SEED, site)).view(M, N).double() * 2.0
        assert 0.3 < (keep > 0).double().mean().item() < 0.7
        val, U, err = val * keep, U * keep, err * keep
    if flags & RES:
        r64 = rvals.double()
        val, U = val + r64, U + r64.abs()
        err = err + _E * U
    got = runs[0].region.double().cpu()
    rows = torch.ones(M, dtype=torch.bool)
    if nan_row is not None:
        assert bool(torch.isnan(got[nan_row]).all()), what + f": row {nan_row} of the output is not all NaN"
        rows[nan_row] = False
    got, val, err, U = got[rows], val[rows], err[rows], U[rows]
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite (unwritten?) elements in range"
    if regime == "integer":
        assert U.max().item() < 2.0 ** 24
        bad = got != val
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ; first {_first_bad(bad)}: got {got[_first_bad(bad)].item()!r} ref {val[_first_bad(bad)].item()!r}"
        return
    bound = 1.01 * err + _ulp(val, F32)
    d = (got - val).abs()
    frac = (d / bound).max().item()
    key = (entry, path)
    _WORST[key] = max(_WORST.get(key, -1.0), frac)
    print(f"frac {what}: {frac:.3f}")
    bad = d > bound
    if bool(bad.any()):
        i = _first_bad(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of bound (worst fraction {frac:.3f}); first {i}: "
                             f"got {got[i].item()!r} ref {val[i].item()!r} allowed {bound[i].item():.3e}")


# ---------------------------------------------------------------------------------------------------------------------------
# tests

@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("M,N,K", F32_SHAPES)
def test_gemm_f32(gpu, M, N, K, regime):
    """every flag set with both ldc"""
    for i, (_, flags, alias) in enumerate(FLAGSETS):
        for pad in LDC_PADS:
            _run("tcavt_gemm_f32", gpu["device"], regime, M, N, K, flags, pad, alias, seed=100 * (M + N + K) + 2 * i + (pad > 0))


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("M,N,K", DROP_SHAPES)
def test_gemm_f32_dropout(gpu, M, N, K, regime):
    """bias -> ReLU -> keep_mask at m * N + n, times 2 -> residual, two sites"""
    for site in (3, 77):
        _run("tcavt_gemm_f32", gpu["device"], regime, M, N, K, BIAS | RELU | RES, 5, False, seed=7 * (M + N + K) + site, dropout=0.5, site=site)


@pytest.mark.parametrize("pad", LDC_PADS)
@pytest.mark.parametrize("M,N,K", NAN_SHAPES)
def test_gemm_f32_nan_row(gpu, M, N, K, pad):
    """one NaN in a row of A, with RELU: that output row is NaN, every other row finite and inside its bound"""
    for flags in (RELU, BIAS | RELU | RES):
        _run("tcavt_gemm_f32", gpu["device"], "realistic", M, N, K, flags, pad, False, seed=11 * (M + N + K) + flags, nan_row=M // 2)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("M,N,K", STRIDED_SHAPES + TIE_SHAPES)
def test_gemm_f32_strided(gpu, M, N, K, regime):
    """the four orientations x (none, ACCUM, BIAS|RESIDUAL, RELU) with an 8-slice workspace"""
    tie = (M, N, K) in TIE_SHAPES
    for oi, (oa, ow) in enumerate(ORIENTS):
        for fi, (_, flags) in enumerate(STRIDED_FLAGS):
            _run("tcavt_gemm_f32_strided", gpu["device"], regime, M, N, K, flags, 0, False, seed=13 * (M + N + K) + 4 * oi + fi,
                 oa=oa, ow=ow, pad=not tie, ws_slices=WS_SLICES)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("M,N,K", STRIDED_SHAPES[1:])
def test_gemm_f32_strided_without_workspace(gpu, M, N, K, regime):
    """ldc == N: two splits through atomics; ldc > N and the residual aliasing C: unsplit"""
    for oi, (oa, ow) in enumerate(ORIENTS):
        for ni, (_, flags, pad, alias) in enumerate(NO_WS):
            _run("tcavt_gemm_f32_strided", gpu["device"], regime, M, N, K, flags, pad, alias, seed=17 * (M + N + K) + 4 * oi + ni, oa=oa, ow=ow)


def test_refusals(gpu):
    dev = gpu["device"]
    d = torch.zeros(256, device=dev).data_ptr()
    C = Guarded(4, 4, F32, dev, ld=4, before=4, after=4)
    L = _L()

    def refused(rc, name, what):
        torch.cuda.synchronize()
        assert rc != 0, f"{what}: accepted"
        assert _last_error().startswith(name + ":"), f"{what}: tcavt_last_error() = {_last_error()!r} does not name {name}"
        assert torch.equal(_bits(C.buf), _bits(C.before)), f"{what}: a refused call wrote to C"

    def f32(A=d, W=d, bias=d, res=d, Cp=C.ptr, M=4, flags=0, p=0.0):
        return L.tcavt_gemm_f32(A, 4, W, 4, bias, res, 4, Cp, 4, M, 4, 4, flags, p, 0, 0, _st())

    def strided(A=d, W=d, bias=d, res=d, Cp=C.ptr, K=4, flags=0):
        return L.tcavt_gemm_f32_strided(A, 4, 1, W, 4, 1, bias, res, 4, Cp, 4, 4, 4, K, flags, None, 0, _st())

    refused(f32(A=None), "gemm_f32", "A NULL")
    refused(f32(W=None), "gemm_f32", "W NULL")
    refused(f32(Cp=None), "gemm_f32", "C NULL")
    refused(f32(M=0), "gemm_f32", "M = 0")
    refused(f32(flags=ACCUM), "gemm_f32", "ACCUM, which only the strided entry takes")
    refused(f32(flags=8), "gemm_f32", "SILU_MUL")
    refused(f32(flags=BIAS, bias=None), "gemm_f32", "BIAS without bias")
    refused(f32(flags=RES, res=None), "gemm_f32", "RESIDUAL without residual")
    refused(f32(p=1.0), "gemm_f32", "dropout_p = 1")
    refused(strided(A=None), "gemm_f32_strided", "A NULL")
    refused(strided(Cp=None), "gemm_f32_strided", "C NULL")
    refused(strided(K=0), "gemm_f32_strided", "K = 0")
    refused(strided(flags=ACCUM | RELU), "gemm_f32_strided", "ACCUM with RELU")
    refused(strided(flags=16), "gemm_f32_strided", "ROPE")
    refused(strided(flags=BIAS, bias=None), "gemm_f32_strided", "BIAS without bias")


def test_report_worst_ratio(gpu):
    """(runs last in file order) prints the worst fraction of the bound measured in this session per entry and path"""
    for k in sorted(_WORST):
        print(f"{k[0]:24s} {k[1]:8s} worst frac {_WORST[k]:7.3f}")
