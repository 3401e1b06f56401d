"""The forward row kernels (csrc/core.hip, csrc/stack.hip) against float64: tcavt_rmsnorm, tcavt_rmsnorm16, tcavt_layernorm,
tcavt_cast_f32_16, tcavt_embed_fuse, tcavt_rownorm_prep.

Every case calls the C entry point (capi.lib().tcavt_*) and checks every element against ONE float64 evaluation of the operation in
torch on the CPU, from the same fp32 / 16-bit input values.  Nothing in a reference comes from a project kernel: dropout masks are
oracle/philox.py keep_mask(M * H, p, seed, site) with element index m * H + n, 1 / (1 - p) is the host's fp32 quotient.

Buffers: every output lies in a larger NaN-filled allocation with guard rows before and after; every in-range element must come back
finite and inside its bound, every guard element keep its bits, every input stay bit-unchanged, a second launch give the same
bits.  Optional outputs run in every combination the entry allows (16-bit only, fp32 only, both), in fp16 and bf16.

Bounds, derived next to each reference (the library is built with -ffp-contract=off: every product and every sum rounds once):
    |got - ref| <= 1.01 * [fp32 terms] + _T * |what rsqrtf scales| + ulp_out(ref)
_T = 4 * 2^-24 for rsqrtf; the fp32 accumulation term is n * 2^-24 * unit, n = the number of terms on the longest summation
chain read from the kernel (the terms a lane adds serially, the 6 exchange levels of wave_sum, the product, the divide, the eps
add).  LayerNorm carries the cancellation term: the error of v - mean scales with |v| and |mean|, not with |y|.  Where an output
is an exact function of another output or of the inputs the test asserts bits: out16 == round(out_f32), out_drop ==
to16(from16(out16) * keep / (1 - p)), the cast, h (one IEEE addition), h16 == round(scale * h), x16, part[:, 1:] == 0, a
16-bit-only or fp32-only call == the same output of the call that writes both.

Cases (test_cases_cover_the_host_rules mirrors each entry's dispatch rule and asserts from these lists that every instantiation
and boundary is reached):

| tcavt_rmsnorm (M, H) | reaches |          | tcavt_rmsnorm16 (M, H) | reaches |
|---|---|                                 |---|---|
| (1, 8) | NV=0, two lanes |              | (1, 256) | tail step only |
| (3, 264) | NV=0, two lanes twice |      | (5, 512) | one full step, no tail |
| (2, 1280) | H / 256 = 5 -> NV=0 |       | (3, 768) | one step plus tail |
| (1, 8192) | the limit, NV=0 |           | (4, 2048) | product width |
| (5, 256) | NV=1, M % 4 != 0 |           | (2, 4096) | eight steps, all in registers |
| (4, 512) (3, 768) (2, 1024) | NV=2, 3, 4 | (2, 4352) | eight steps plus tail |
| (6, 2048) | NV=8, product width |       | (3, 4608) | the ninth step streams (i >= NV) |
| (2, 4096) | NV=16 |                     | (1, 8192) | the limit |
gamma has a per-column pattern that is never 1 and never repeats.  Planted rows (every shape sees all of them, over several calls
where M < 5): all zero (output exactly 0), |x| ~ 1e-3 (eps decides), one spike of 1e4 among zeros, a row times 1e4.
out_drop at p = 0.1 and 0.5.

| tcavt_layernorm (M, D) | reaches |
|---|---|
| (1, 4) | smallest D |   (5, 64) product width | (3, 256) nvec = 64, the last NV=1 | (3, 260) the first NV=4, one lane twice |
| (50, 768) | product width | (2, 1024) the last NV=4 | (2, 1028) the first NV=16 | (1, 4096) the limit |
Residual given and NULL.  Planted rows: constant (y = beta up to the bound), 1000 + N(0, 1), a residual that cancels x to ~1e-3.
test_layernorm_formula_matches_torch ties the closed form to torch.nn.functional.layer_norm in float64 (1e-12 relative).

tcavt_cast_f32_16: n = 1, 7, 8, 9, 1003, 8 * 256 * 4096 + 8 * 300 + 5 (a second grid-stride round, a partial last round, a tail), bit
for bit against x.cpu().to(dtype), with ties both ways, the largest finite value and the first value that rounds to inf, subnormals,
values that round to 0, +-0, +-inf and NaN at known indices, the tail included.

| tcavt_embed_fuse (B, Nq, Lt, H, V) | reaches |        | tcavt_rownorm_prep (M, H) | reaches |
|---|---|                                              |---|---|
| (1, 0, 1, 8, 3) | text only |                         | (1, 4) | smallest |
| (1, 1, 0, 8, 3) | image only |                        | (5, 256) | M % 4 != 0 |
| (3, 4, 9, 256, 50) | the earlier test's shape |       | (3, 260) | one lane takes a second round |
| (5, 3, 2, 264, 7) | rows % 4 != 0, partial steps |    | (6, 2048) | product width |
| (2, 16, 5, 2048, 1000) | product width and Nq |
embed_fuse modes: h only, h with h16 / part, h == NULL; table fp16 / bf16; stream_scale 0 (meaning 1), 1, 0.25; npart 1, 4, H / 64, 70.
Ids -1, V and 2^40 each set the flag and yield row 0 of the table.  rownorm_prep: rounded_sums 0 / 1, scale 1 / 0.25, npart 1 / 4 / 70.

Refusals pass only arguments that the host code rejects before any launch (read from the entry points): non-zero status,
tcavt_last_error names the entry, the outputs keep their bits.

MEASURED on an MI355X: the worst fraction of the whole bound per (entry point, instantiation, type) stands beside the constants
below; profiles/forward_kernels_bounds.txt has every line, test_report_worst_ratio prints the session's (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch

from test_attention_bwd_gpu import _first_bad, _last_error, _name, _same_bits
from test_gemm_forms_gpu import Poisoned, _bits, _dt_code, _round, _ulp
from test_llm_backward_kernels_gpu import EPS, SEED, Guarded, _gen, _inv_keep, _L, _ok, _st, _unchanged

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
DTYPES = [F16, BF16]
_E = 2.0 ** -24   # unit roundoff of fp32
_T = 4 * _E       # rsqrtf: 2 ulps of the result (the project's constant)
SITE = 77
# MEASURED on an MI355X: worst fraction of the whole bound (bar 1.0) over the cases, fp16 | bf16 (profiles/forward_kernels_bounds.txt
# has every instantiation).  0.5 = the output rounding alone (half of the output ulp the bound allows); fp32 outputs lie far below
# it where the bound is the worst-case summation chain.
#   tcavt_rmsnorm      rmsnorm_kernel<NV=0>                         out16 0.499 | 0.500   out_f32 0.150 | 0.150
#   tcavt_rmsnorm      rmsnorm_kernel<NV=16>                        out16 0.498 | 0.500   out_f32 0.060 | 0.060
#   tcavt_rmsnorm      rmsnorm_kernel<NV=1>                         out16 0.499 | 0.499   out_f32 0.172 | 0.172
#   tcavt_rmsnorm      rmsnorm_kernel<NV=2>                         out16 0.499 | 0.500   out_f32 0.124 | 0.124
#   tcavt_rmsnorm      rmsnorm_kernel<NV=3>                         out16 0.499 | 0.500   out_f32 0.133 | 0.133
#   tcavt_rmsnorm      rmsnorm_kernel<NV=4>                         out16 0.499 | 0.500   out_f32 0.117 | 0.117
#   tcavt_rmsnorm      rmsnorm_kernel<NV=8>                         out16 0.499 | 0.500   out_f32 0.092 | 0.092
#   tcavt_rmsnorm16    rmsnorm16_kernel steps=0+0 tail=1            out16 0.499 | 0.499   out_f32 0.145 | 0.157
#   tcavt_rmsnorm16    rmsnorm16_kernel steps=1+0 tail=0            out16 0.499 | 0.500   out_f32 0.147 | 0.131
#   tcavt_rmsnorm16    rmsnorm16_kernel steps=1+0 tail=1            out16 0.499 | 0.500   out_f32 0.121 | 0.138
#   tcavt_rmsnorm16    rmsnorm16_kernel steps=4+0 tail=0            out16 0.499 | 0.500   out_f32 0.088 | 0.090
#   tcavt_rmsnorm16    rmsnorm16_kernel steps=8+0 tail=0            out16 0.498 | 0.500   out_f32 0.057 | 0.047
#   tcavt_rmsnorm16    rmsnorm16_kernel steps=8+0 tail=1            out16 0.498 | 0.500   out_f32 0.064 | 0.061
#   tcavt_rmsnorm16    rmsnorm16_kernel steps=8+1 tail=0            out16 0.498 | 0.500   out_f32 0.073 | 0.069
#   tcavt_rmsnorm16    rmsnorm16_kernel steps=8+8 tail=0            out16 0.498 | 0.500   out_f32 0.032 | 0.046
#   tcavt_layernorm    layernorm_kernel<NV=16>                      out16 0.498 | 0.500   out_f32 0.081 | 0.081
#   tcavt_layernorm    layernorm_kernel<NV=16> residual             out16 0.497 | 0.500   out_f32 0.060 | 0.060
#   tcavt_layernorm    layernorm_kernel<NV=1>                       out16 0.500 | 0.499   out_f32 0.154 | 0.154
#   tcavt_layernorm    layernorm_kernel<NV=1> residual              out16 0.499 | 0.498   out_f32 0.105 | 0.105
#   tcavt_layernorm    layernorm_kernel<NV=4>                       out16 0.499 | 0.500   out_f32 0.126 | 0.126
#   tcavt_layernorm    layernorm_kernel<NV=4> residual              out16 0.499 | 0.500   out_f32 0.118 | 0.118
#   tcavt_embed_fuse   embed_fuse_kernel part                       part  0.126 | 0.126
#   tcavt_embed_fuse   embed_fuse_kernel part (h == NULL: rounded values) part  0.134 | 0.130
#   tcavt_rownorm_prep rownorm_prep_kernel                          part  0.105 | 0.130
#   tcavt_rownorm_prep rownorm_prep_kernel rounded sums             part  0.135 | 0.132
# Mutants (profiles/forward_kernels_bounds.txt): the last vector of rmsnorm_kernel<3> left out of the sum, the NV=0 form summing a
# lane's first round only, eps dropped, rmsnorm16 without its tail step / with the streamed sum starting at NV + 1, LayerNorm
# dividing by D - 1 / skipping the residual from idx 64 on, embed_fuse adding m0 to both halves / summing unrounded values with
# h == NULL, part written for k < 64 only, the cast dropping the last tail element, out_drop indexed by row * H + idx: each
# fails here; the earlier tests pass the first three and the tenth.
_WORST = {}   # (entry, instantiation, type) -> worst fraction


def _record(key, frac):
    _WORST[key] = max(_WORST.get(key, -1.0), frac)


def _check(got, ref, bound, what, key):
    """|got - ref| <= bound per element (float64, CPU); every element finite; records the worst fraction of the bound"""
    g = got.double().cpu()
    assert torch.isfinite(g).all(), f"{what}: {int((~torch.isfinite(g)).sum())} non-finite (unwritten?) elements in range"
    d = (g - ref).abs()
    frac = (d / bound.clamp_min(1e-300)).max().item()
    _record(key, frac)
    print(f"frac {what}: {frac:.3f}")
    bad = d > bound
    if bool(bad.any()):
        i = _first_bad(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of bound (worst fraction {frac:.3f}); first {i}: "
                             f"got {g[i].item()!r} ref {ref[i].item()!r} allowed {bound[i].item():.3e}")


def _guarded(rows, cols, dt, dev, fill=None):
    """a Guarded [rows, cols] with at least three guard rows on each side (as many as keep the region 16-byte aligned)"""
    size = 4 if dt in (F32, torch.int32) else 2
    k = next(k for k in range(3, 12) if (k * cols * size) % 16 == 0)
    return Guarded(rows, cols, dt, dev, fill=fill, before=k, after=k)


def _untouched(bufs, what):
    for b in bufs:
        assert torch.equal(_bits(b.buf), _bits(b.before)), f"{what}: a refused call wrote to an output"


def _refused(rc, name, bufs, what):
    """a refusal: non-zero status, tcavt_last_error names the entry, the outputs keep their bits"""
    torch.cuda.synchronize()
    assert rc != 0, f"{what}: accepted"
    assert _last_error().startswith(name + ":"), f"{what}: tcavt_last_error() = {_last_error()!r} does not name {name}"
    _untouched(bufs, what)


def _bits_equal(got, want, what):
    bad = _bits(got.contiguous().cpu()) != _bits(want.contiguous().cpu())
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ in bits; first {_first_bad(bad)}"


def _gamma(n, dev, lo=0.75):
    """per column, never 1, no two columns alike (37 h mod the prime 8209 is one-to-one below 8209)"""
    h = torch.arange(n, dtype=F64)
    g = (lo + ((h * 37) % 8209) / 8209).float()
    assert bool((g != 1).all())
    return g.to(dev)


@functools.lru_cache(maxsize=None)
def _keep_np(n, p, site):
    from oracle.philox import keep_mask

    return keep_mask(n, p, SEED, site)


def _keep_scale(M, H, p, site):
    """fp32 [M, H] on the CPU: 1 / (1 - p) (the host's fp32 quotient) where the oracle keeps element m * H + n, else 0"""
    keep = torch.from_numpy(_keep_np(M * H, p, site).astype(np.float32)).view(M, H)
    return keep * torch.tensor(_inv_keep(p), dtype=F32)


# ---------------------------------------------------------------------------------------------------------------------------
# case lists and the host rules

RMS_CASES = [(1, 8), (3, 264), (2, 1280), (1, 8192), (5, 256), (4, 512), (3, 768), (2, 1024), (6, 2048), (2, 4096)]
RMS16_CASES = [(1, 256), (5, 512), (3, 768), (4, 2048), (2, 4096), (2, 4352), (3, 4608), (1, 8192)]
LN_CASES = [(1, 4), (5, 64), (3, 256), (3, 260), (50, 768), (2, 1024), (2, 1028), (1, 4096)]
CAST_N = [1, 7, 8, 9, 1003, 8 * 256 * 4096 + 8 * 300 + 5]
EMBED_CASES = [(1, 0, 1, 8, 3), (1, 1, 0, 8, 3), (3, 4, 9, 256, 50), (5, 3, 2, 264, 7), (2, 16, 5, 2048, 1000)]
# (h given, h16 / part given, stream_scale, npart; "H/64" where H >= 64, else 1)
EMBED_CALLS = [(1, 0, 0.0, 0), (1, 1, 0.0, 1), (1, 1, 0.25, 4), (1, 1, 1.0, "H/64"), (1, 1, 0.25, 70),
               (0, 1, 0.0, 4), (0, 1, 0.25, 70), (0, 1, 1.0, 1), (0, 1, 0.25, "H/64")]
PREP_CASES = [(1, 4), (5, 256), (3, 260), (6, 2048)]
PREP_CALLS = [(r, s, n) for r in (0, 1) for s in (1.0, 0.25) for n in (1, 4, 70)]
N_PATTERNS_RMS, N_PATTERNS_LN = 5, 4


def _rms_nv(H):
    """the instantiation tcavt_rmsnorm launches: NV float4 per lane, 0 = the two-pass form"""
    return H // 256 if H % 256 == 0 and H // 256 in (1, 2, 3, 4, 8, 16) else 0


def _rms_terms(H):
    """squares a lane adds serially in rmsnorm_kernel: four per float4, ceil(H / 4 / 64) float4 for lane 0"""
    return 4 * -(-(H // 4) // 64)


def _rms16_steps(H):
    """(512-column steps in registers, steps streamed by the i >= NV loop, tail step of 256 columns) of rmsnorm16_kernel"""
    nv = H // 512
    return min(nv, 8), max(nv - 8, 0), int(H % 512 != 0)


def _rms16_terms(H):
    reg, streamed, tail = _rms16_steps(H)
    return 8 * (reg + streamed) + 4 * tail


def _ln_nv(D):
    nvec = D // 4
    return 1 if nvec <= 64 else 4 if nvec <= 256 else 16


def _cast_grid(n):
    """(blocks, whole grid-stride rounds, octets of a partial last round, tail elements) of tcavt_cast_f32_16"""
    blocks = min(max((n // 8 + 255) // 256, 1), 4096)
    return blocks, (n // 8) // (blocks * 256), (n // 8) % (blocks * 256), n % 8


def _npart(n, H):
    return max(H // 64, 1) if n == "H/64" else n


def _shifts(M, n_patterns):
    """row i of call `shift` holds pattern (i + shift) % n_patterns: over these calls every row pattern appears"""
    return range(0, n_patterns, M)


def test_cases_cover_the_host_rules():
    """from the case lists alone (the host arithmetic of the entry points mirrored): every instantiation and every edge is reached"""
    # rmsnorm: H % 256 == 0 with H / 256 in {1, 2, 3, 4, 8, 16} -> NV = H / 256, else the two-pass form; four rows per block
    assert sorted(_rms_nv(H) for _, H in RMS_CASES) == [0, 0, 0, 0, 1, 2, 3, 4, 8, 16]
    nv0 = [(M, H) for M, H in RMS_CASES if _rms_nv(H) == 0]
    assert any(H // 4 == 2 for _, H in nv0)                                   # two lanes
    assert any(64 < H // 4 < 128 and H // 4 - 64 == 2 for _, H in nv0)        # two lanes take a second round
    assert any(H % 256 == 0 and H // 256 == 5 for _, H in nv0)                # a multiple of 256 without an instantiation
    assert any(H == 8192 for _, H in nv0) and all(H <= 8192 and H % 8 == 0 for _, H in RMS_CASES)
    assert any(M % 4 and _rms_nv(H) == 1 for M, H in RMS_CASES) and (6, 2048) in RMS_CASES
    assert _rms_terms(8) == 4 and _rms_terms(264) == 8 and _rms_terms(2048) == 32 and _rms_terms(8192) == 128
    for M, _ in RMS_CASES + RMS16_CASES:   # every planted row pattern reaches every shape
        assert {(i + s) % N_PATTERNS_RMS for s in _shifts(M, N_PATTERNS_RMS) for i in range(M)} == set(range(N_PATTERNS_RMS))
    # rmsnorm16: H % 256 == 0; H / 512 whole steps (eight in registers, the others streamed), one 256-column tail step
    assert [_rms16_steps(H) for _, H in RMS16_CASES] == [(0, 0, 1), (1, 0, 0), (1, 0, 1), (4, 0, 0), (8, 0, 0), (8, 0, 1), (8, 1, 0), (8, 8, 0)]
    assert all(H % 256 == 0 for _, H in RMS16_CASES) and any(M % 4 for M, _ in RMS16_CASES)
    # layernorm: nvec = D / 4 <= 64 -> NV=1, <= 256 -> NV=4, else NV=16; D <= 4096
    assert [(_ln_nv(D), D // 4) for _, D in LN_CASES] == [(1, 1), (1, 16), (1, 64), (4, 65), (4, 192), (4, 256), (16, 257), (16, 1024)]
    assert any(M % 4 for M, _ in LN_CASES) and (5, 64) in LN_CASES and (50, 768) in LN_CASES
    for M, _ in LN_CASES:
        assert {(i + s) % N_PATTERNS_LN for s in _shifts(M, N_PATTERNS_LN) for i in range(M)} == set(range(N_PATTERNS_LN))
    # cast: octets over at most 4096 blocks of 256 threads, n % 8 tail elements by the first threads
    assert [_cast_grid(n) for n in CAST_N] == [(1, 0, 0, 1), (1, 0, 0, 7), (1, 0, 1, 0), (1, 0, 1, 1), (1, 0, 125, 3), (4096, 1, 300, 5)]
    # embed_fuse: one wave per row, four rows per block; 256 columns per image step, 512 per text step
    shapes = {(B * (Nq + Lt), Nq > 0, Lt > 0, H) for B, Nq, Lt, H, _ in EMBED_CASES}
    assert any(not q and t for _, q, t, _ in shapes) and any(q and not t for _, q, t, _ in shapes)
    assert (3, 4, 9, 256, 50) in EMBED_CASES and any(r % 4 and H % 256 and H % 512 for r, _, _, H in shapes)
    assert any(H == 2048 and Nq == 16 for _, Nq, _, H, _ in EMBED_CASES) and all(H % 8 == 0 for *_, H, _ in EMBED_CASES)
    assert {(h, w) for h, w, _, _ in EMBED_CALLS} == {(1, 0), (1, 1), (0, 1)}
    for h in (0, 1):
        assert {s for hh, w, s, _ in EMBED_CALLS if w and hh == h} == {0.0, 0.25, 1.0}
        assert {_npart(n, 2048) for hh, w, _, n in EMBED_CALLS if w and hh == h} == {1, 4, 32, 70}   # 70: a second round of the k loop
    # rownorm_prep: 256 columns per step
    assert [(M % 4, -(-(H // 4) // 64), (H // 4) % 64) for M, H in PREP_CASES] == [(1, 1, 1), (1, 1, 0), (3, 2, 1), (2, 8, 0)]
    assert len(set(PREP_CALLS)) == 12


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_rmsnorm, tcavt_rmsnorm16

def _rms_rows(M, H, shift, g_, spread):
    """float64 [M, H]: row i holds pattern (i + shift) % 5: 0 N(0, 1) with a row gain, 1 all zero, 2 |x| ~ 1e-3, 3 one spike of 1e4
    among zeros, 4 a row times 1e4 (clamped to +-6e4, inside the fp16 range)"""
    x = torch.randn(M, H, generator=g_).double() * spread
    for i in range(M):
        pat = (i + shift) % N_PATTERNS_RMS
        if pat == 0:
            x[i] *= 2.0 ** ((i % 5) - 2)
        elif pat == 1:
            x[i] = 0
        elif pat == 2:
            x[i] *= 1e-3 / spread
        elif pat == 3:
            x[i] = 0
            x[i, (H // 3 + 5 * i) % H] = 1e4
        else:
            x[i] = (x[i] / spread).clamp(-6, 6) * 1e4
    return x


def _rms_ref(x, gamma, terms, out_dt):
    """y = x r gamma, r = 1 / sqrt(mean(x^2) + eps), in float64, and the bound.

    The kernel: every square rounds (E), a lane adds `terms` of them, six exchange levels, the divide by H, the eps add: the
    argument of rsqrtf is a sum of non-negative terms with relative error <= n E, n = terms + 6 + 3; half of it under the root;
    rsqrtf itself _T; two products (x * rs, * gamma): 2 E."""
    r = 1 / torch.sqrt((x * x).mean(1, keepdim=True) + EPS)
    ref = x * r * gamma[None, :]
    n = terms + 6 + 3
    return ref, 1.01 * (0.5 * n + 2) * _E * ref.abs() + _T * ref.abs() + _ulp(ref, out_dt)


def _planted_asserts(x, shift, got, what):
    for i in range(x.shape[0]):
        if (i + shift) % N_PATTERNS_RMS == 1:
            assert bool((got[i].float() == 0).all()), f"{what}: the all-zero row {i} is not exactly 0"


def _rms_run(dev, M, H, dt, shift):
    nv = _rms_nv(H)
    g_ = _gen(1000 + H + shift)
    X = Poisoned(M, H, F32, dev, ld=H, extra_rows=3, fill=_rms_rows(M, H, shift, g_, 3.0))
    gam = _gamma(H, dev)
    gam0 = gam.clone()
    x64, g64 = X.region.double().cpu(), gam.double().cpu()
    what = f"rmsnorm {M}x{H} NV={nv} {_name(dt)} shift={shift}"
    key = ("tcavt_rmsnorm", f"rmsnorm_kernel<NV={nv}>", _name(dt))
    ref, bound32 = _rms_ref(x64, g64, _rms_terms(H), F32)
    _, bound16 = _rms_ref(x64, g64, _rms_terms(H), dt)

    def call(o16, o32, od, p, tag):
        rc = _L().tcavt_rmsnorm(X.buf.data_ptr(), gam.data_ptr(), EPS, o16.ptr if o16 else None, o32.ptr if o32 else None, M, H,
                                od.ptr if od else None, p, SEED, SITE, _dt_code(dt), _st())
        _ok(rc, f"{what} {tag}")
        for o in (o16, o32, od):
            if o:
                o.check(f"{what} {tag}")
        _unchanged([("x", X.buf, X.before), ("gamma", gam, gam0)], f"{what} {tag}")

    def drop_check(o16, od, p, tag):
        want = (o16.region.float().cpu() * _keep_scale(M, H, p, SITE)).to(dt)
        _bits_equal(od.region, want, f"{what} {tag}: out_drop != to16(from16(out16) * keep / (1 - p))")

    # both outputs, out_drop at p = 0.1
    a16, a32, ad = _guarded(M, H, dt, dev), _guarded(M, H, F32, dev), _guarded(M, H, dt, dev)
    call(a16, a32, ad, 0.1, "both")
    _check(a32.region, ref, bound32, what + " out_f32", key + ("f32",))
    _check(a16.region, ref, bound16, what + " out16", key + ("16",))
    _bits_equal(a16.region, _round(a32.region, dt), what + ": out16 != round(out_f32)")
    drop_check(a16, ad, 0.1, "both")
    _planted_asserts(x64, shift, a32.region, what)
    _planted_asserts(x64, shift, a16.region, what)
    # the same call again: the same bits
    b16, b32, bd = _guarded(M, H, dt, dev), _guarded(M, H, F32, dev), _guarded(M, H, dt, dev)
    call(b16, b32, bd, 0.1, "again")
    assert _same_bits(b16.region, a16.region) and _same_bits(b32.region, a32.region) and _same_bits(bd.region, ad.region), what + ": not reproducible"
    # 16-bit only, out_drop at p = 0.5
    c16, cd = _guarded(M, H, dt, dev), _guarded(M, H, dt, dev)
    call(c16, None, cd, 0.5, "16-bit only")
    _check(c16.region, ref, bound16, what + " out16 alone", key + ("16",))
    assert _same_bits(c16.region, a16.region), what + ": out16 alone differs from out16 beside out_f32"
    drop_check(c16, cd, 0.5, "16-bit only")
    # fp32 only
    d32 = _guarded(M, H, F32, dev)
    call(None, d32, None, 0.0, "fp32 only")
    _check(d32.region, ref, bound32, what + " out_f32 alone", key + ("f32",))
    assert _same_bits(d32.region, a32.region), what + ": out_f32 alone differs from out_f32 beside out16"


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("M,H", RMS_CASES)
def test_rmsnorm(gpu, M, H, dt):
    for shift in _shifts(M, N_PATTERNS_RMS):
        _rms_run(gpu["device"], M, H, dt, shift)


def test_rmsnorm_refusals(gpu):
    """read from tcavt_rmsnorm: H % 8, H <= 8192, out_drop needs 0 < p < 1, dtype16, an output, the alignment of what the kernel
    reads and writes with 8- and 16-byte accesses -- all before the launch"""
    dev = gpu["device"]
    H = 256
    x, gam = torch.randn(2, 8200, device=dev), _gamma(8200, dev)
    o16, o32, od = _guarded(2, 8200, BF16, dev), _guarded(2, 8200, F32, dev), _guarded(2, 8200, BF16, dev)
    outs = [o16, o32, od]

    def call(H=H, x=x.data_ptr(), g=gam.data_ptr(), p16=o16.ptr, p32=o32.ptr, pd=None, p=0.0, dtype=_dt_code(BF16)):
        return _L().tcavt_rmsnorm(x, g, EPS, p16, p32, 2, H, pd, p, SEED, SITE, dtype, _st())

    _refused(call(H=12), "rmsnorm", outs, "H = 12")
    _refused(call(H=8200), "rmsnorm", outs, "H = 8200 > 8192")
    _refused(call(pd=od.ptr, p=0.0), "rmsnorm", outs, "out_drop with p = 0")
    _refused(call(pd=od.ptr, p=1.0), "rmsnorm", outs, "p = 1")
    _refused(call(p=1.0), "rmsnorm", outs, "p = 1 without out_drop")
    _refused(call(dtype=7), "rmsnorm", outs, "dtype16 = 7")
    _refused(call(dtype=_dt_code(F32)), "rmsnorm", outs, "dtype16 = TCAVT_F32")
    _refused(call(p16=None, p32=None), "rmsnorm", outs, "both outputs NULL")
    _refused(call(x=x.data_ptr() + 4), "rmsnorm", outs, "x off by 4 bytes")
    _refused(call(g=gam.data_ptr() + 8), "rmsnorm", outs, "gamma off by 8 bytes")
    _refused(call(p16=o16.ptr + 2), "rmsnorm", outs, "out16 off by 2 bytes")
    _refused(call(p16=o16.ptr + 4), "rmsnorm", outs, "out16 off by 4 bytes")
    _refused(call(p32=o32.ptr + 8), "rmsnorm", outs, "out_f32 off by 8 bytes")
    _refused(call(pd=od.ptr + 4, p=0.5), "rmsnorm", outs, "out_drop off by 4 bytes")


def _rms16_run(dev, M, H, dt, shift):
    g_ = _gen(2000 + H + shift)
    X = Poisoned(M, H, dt, dev, ld=H, extra_rows=3, fill=_rms_rows(M, H, shift, g_, 1.0))
    gam = _gamma(H, dev)
    gam0 = gam.clone()
    x64, g64 = X.region.double().cpu(), gam.double().cpu()
    assert torch.isfinite(x64).all()
    reg, streamed, tail = _rms16_steps(H)
    what = f"rmsnorm16 {M}x{H} steps={reg}+{streamed} tail={tail} {_name(dt)} shift={shift}"
    key = ("tcavt_rmsnorm16", f"rmsnorm16_kernel steps={reg}+{streamed} tail={tail}", _name(dt))
    ref, bound32 = _rms_ref(x64, g64, _rms16_terms(H), F32)
    _, bound16 = _rms_ref(x64, g64, _rms16_terms(H), dt)

    def call(o16, o32, tag):
        rc = _L().tcavt_rmsnorm16(X.buf.data_ptr(), gam.data_ptr(), EPS, o16.ptr if o16 else None, o32.ptr if o32 else None, M, H,
                                  _dt_code(dt), _st())
        _ok(rc, f"{what} {tag}")
        for o in (o16, o32):
            if o:
                o.check(f"{what} {tag}")
        _unchanged([("x16", X.buf, X.before), ("gamma", gam, gam0)], f"{what} {tag}")

    a16, a32 = _guarded(M, H, dt, dev), _guarded(M, H, F32, dev)
    call(a16, a32, "both")
    _check(a32.region, ref, bound32, what + " out_f32", key + ("f32",))
    _check(a16.region, ref, bound16, what + " out16", key + ("16",))
    _bits_equal(a16.region, _round(a32.region, dt), what + ": out16 != round(out_f32)")
    _planted_asserts(x64, shift, a32.region, what)
    _planted_asserts(x64, shift, a16.region, what)
    b16, b32 = _guarded(M, H, dt, dev), _guarded(M, H, F32, dev)
    call(b16, b32, "again")
    assert _same_bits(b16.region, a16.region) and _same_bits(b32.region, a32.region), what + ": not reproducible"
    c16, d32 = _guarded(M, H, dt, dev), _guarded(M, H, F32, dev)
    call(c16, None, "16-bit only")
    call(None, d32, "fp32 only")
    _check(c16.region, ref, bound16, what + " out16 alone", key + ("16",))
    _check(d32.region, ref, bound32, what + " out_f32 alone", key + ("f32",))
    assert _same_bits(c16.region, a16.region) and _same_bits(d32.region, a32.region), what + ": an output alone differs from the pair"


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("M,H", RMS16_CASES)
def test_rmsnorm16(gpu, M, H, dt):
    for shift in _shifts(M, N_PATTERNS_RMS):
        _rms16_run(gpu["device"], M, H, dt, shift)


def test_rmsnorm16_refusals(gpu):
    dev = gpu["device"]
    x, gam = torch.randn(2, 512, device=dev).to(F16), _gamma(512, dev)
    o16, o32 = _guarded(2, 512, F16, dev), _guarded(2, 512, F32, dev)
    outs = [o16, o32]

    def call(H=256, x=x.data_ptr(), g=gam.data_ptr(), p16=o16.ptr, p32=o32.ptr, dtype=_dt_code(F16)):
        return _L().tcavt_rmsnorm16(x, g, EPS, p16, p32, 2, H, dtype, _st())

    _refused(call(H=264), "rmsnorm16", outs, "H = 264")
    _refused(call(dtype=_dt_code(F32)), "rmsnorm16", outs, "dtype16 = TCAVT_F32")
    _refused(call(p16=None, p32=None), "rmsnorm16", outs, "both outputs NULL")
    _refused(call(x=x.data_ptr() + 8), "rmsnorm16", outs, "x16 off by 8 bytes")
    _refused(call(p16=o16.ptr + 8), "rmsnorm16", outs, "out16 off by 8 bytes")
    _refused(call(p32=o32.ptr + 8), "rmsnorm16", outs, "out_f32 off by 8 bytes")


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_layernorm

def _ln_rows(M, D, shift, with_res, g_):
    """float64 x, residual [M, D]: row i holds pattern (i + shift) % 4: 0 N(0, 1) with a row gain, 1 a constant row, 2 a row at
    1000 + N(0, 1), 3 a residual that cancels x to ~1e-3 (without a residual: x ~ 1e-3)"""
    x = torch.randn(M, D, generator=g_).double()
    res = torch.randn(M, D, generator=g_).double()
    for i in range(M):
        pat = (i + shift) % N_PATTERNS_LN
        if pat == 0:
            x[i] *= 2.0 ** ((i % 5) - 2)
        elif pat == 1:
            x[i], res[i] = 2.5 + i, 0.75
        elif pat == 2:
            x[i], res[i] = x[i] + 1000, res[i] * 0.5
        else:
            res[i] = -x[i].float().double() + 1e-3 * res[i]
            if not with_res:
                x[i] *= 1e-3
    return x, res


def _ln_ref(x, res, gamma, beta, D, out_dt):
    """y = (v - mean) r gamma + beta, v = x + residual, r = 1 / sqrt(var + eps) (biased variance), in float64, and the bound.

    terms = 4 * ceil(D / 4 / 64) values a lane adds serially.  v: one addition, dv = E |v| (none without a residual).
    mean: n_s = terms + 6 + 1 (the divide) on mean|v|, plus the mean of dv: dmean.  d = v - mean: the CANCELLATION term
    dd = E (|v| + |mean|) + dmean + dv -- it scales with |v| and |mean|, not with |d|.  var = mean(d^2): n_q = terms + 6 + 3 (the
    square, the divide, the eps add) relative on var, and what dd brings: 2 mean(|d| dd) + mean(dd^2).  r: half of that relative to
    var + eps, and rsqrtf (_T, on |d r gamma|).  y: two products (2 E on |d r gamma|), dd r |gamma|, the addition of beta (E |y|)."""
    v = x + res if res is not None else x
    terms = 4 * -(-(D // 4) // 64)
    a = v.abs().mean(1, keepdim=True)
    mean = v.mean(1, keepdim=True)
    dv = _E * v.abs() if res is not None else 0 * v
    dmean = (terms + 6 + 1) * _E * a + (_E * a if res is not None else 0)
    d = v - mean
    dd = _E * (v.abs() + mean.abs()) + dmean + dv
    var = (d * d).mean(1, keepdim=True)
    dvar = (terms + 6 + 3) * _E * (var + EPS) + 2 * (d.abs() * dd).mean(1, keepdim=True) + (dd * dd).mean(1, keepdim=True)
    r = 1 / torch.sqrt(var + EPS)
    drg = d * r * gamma[None, :]
    ref = drg + beta[None, :]
    f32 = drg.abs() * (0.5 * dvar / (var + EPS) + 2 * _E) + dd * r * gamma.abs()[None, :] + _E * ref.abs()
    return ref, 1.01 * f32 + _T * drg.abs() + _ulp(ref, out_dt)


def test_layernorm_formula_matches_torch():
    g_ = _gen(11)
    x, res = _ln_rows(7, 260, 0, True, g_)
    gamma, beta = torch.randn(260, generator=g_).double(), torch.randn(260, generator=g_).double()
    ref, _ = _ln_ref(x, res, gamma, beta, 260, F32)
    want = torch.nn.functional.layer_norm(x + res, (260,), gamma, beta, EPS)
    assert ((ref - want).norm() / want.norm()).item() < 1e-12


def _ln_run(dev, M, D, dt, with_res, shift):
    g_ = _gen(3000 + D + shift)
    x, res = _ln_rows(M, D, shift, with_res, g_)
    X = Poisoned(M, D, F32, dev, ld=D, extra_rows=3, fill=x)
    R = Poisoned(M, D, F32, dev, ld=D, extra_rows=3, fill=res) if with_res else None
    gam, bet = _gamma(D, dev), _gamma(D, dev, lo=-0.5).flip(0).contiguous()
    gam0, bet0 = gam.clone(), bet.clone()
    nv = _ln_nv(D)
    what = f"layernorm {M}x{D} NV={nv} {_name(dt)} residual={with_res} shift={shift}"
    key = ("tcavt_layernorm", f"layernorm_kernel<NV={nv}>" + (" residual" if with_res else ""), _name(dt))
    x64, r64 = X.region.double().cpu(), R.region.double().cpu() if with_res else None
    ref, bound32 = _ln_ref(x64, r64, gam.double().cpu(), bet.double().cpu(), D, F32)
    _, bound16 = _ln_ref(x64, r64, gam.double().cpu(), bet.double().cpu(), D, dt)

    def call(o32, o16, tag):
        rc = _L().tcavt_layernorm(X.buf.data_ptr(), R.buf.data_ptr() if with_res else None, gam.data_ptr(), bet.data_ptr(), EPS,
                                  o32.ptr if o32 else None, o16.ptr if o16 else None, M, D, _dt_code(dt), _st())
        _ok(rc, f"{what} {tag}")
        for o in (o16, o32):
            if o:
                o.check(f"{what} {tag}")
        pairs = [("x", X.buf, X.before), ("gamma", gam, gam0), ("beta", bet, bet0)]
        if with_res:
            pairs.append(("residual", R.buf, R.before))
        _unchanged(pairs, f"{what} {tag}")

    a16, a32 = _guarded(M, D, dt, dev), _guarded(M, D, F32, dev)
    call(a32, a16, "both")
    _check(a32.region, ref, bound32, what + " out_f32", key + ("f32",))
    _check(a16.region, ref, bound16, what + " out16", key + ("16",))
    _bits_equal(a16.region, _round(a32.region, dt), what + ": out16 != round(out_f32)")
    b16, b32 = _guarded(M, D, dt, dev), _guarded(M, D, F32, dev)
    call(b32, b16, "again")
    assert _same_bits(b16.region, a16.region) and _same_bits(b32.region, a32.region), what + ": not reproducible"
    c16, d32 = _guarded(M, D, dt, dev), _guarded(M, D, F32, dev)
    call(None, c16, "16-bit only")
    call(d32, None, "fp32 only")
    _check(c16.region, ref, bound16, what + " out16 alone", key + ("16",))
    _check(d32.region, ref, bound32, what + " out_f32 alone", key + ("f32",))
    assert _same_bits(c16.region, a16.region) and _same_bits(d32.region, a32.region), what + ": an output alone differs from the pair"


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("M,D", LN_CASES)
def test_layernorm(gpu, M, D, dt, with_res):
    for shift in _shifts(M, N_PATTERNS_LN):
        _ln_run(gpu["device"], M, D, dt, with_res, shift)


def test_layernorm_refusals(gpu):
    dev = gpu["device"]
    x, r = torch.randn(2, 4100, device=dev), torch.randn(2, 4100, device=dev)
    gam, bet = _gamma(4100, dev), _gamma(4100, dev)
    o32, o16 = _guarded(2, 4100, F32, dev), _guarded(2, 4100, BF16, dev)
    outs = [o32, o16]

    def call(D=64, x=x.data_ptr(), r=r.data_ptr(), g=gam.data_ptr(), b=bet.data_ptr(), p32=o32.ptr, p16=o16.ptr, dtype=_dt_code(BF16)):
        return _L().tcavt_layernorm(x, r, g, b, EPS, p32, p16, 2, D, dtype, _st())

    _refused(call(D=6), "layernorm", outs, "D = 6")
    _refused(call(D=4100), "layernorm", outs, "D = 4100")
    _refused(call(p32=None, p16=None), "layernorm", outs, "both outputs NULL")
    _refused(call(dtype=_dt_code(F32)), "layernorm", outs, "dtype16 = TCAVT_F32")
    _refused(call(x=x.data_ptr() + 4), "layernorm", outs, "x off by 4 bytes")
    _refused(call(r=r.data_ptr() + 8), "layernorm", outs, "residual off by 8 bytes")
    _refused(call(g=gam.data_ptr() + 4), "layernorm", outs, "gamma off by 4 bytes")
    _refused(call(b=bet.data_ptr() + 4), "layernorm", outs, "beta off by 4 bytes")
    _refused(call(p32=o32.ptr + 8), "layernorm", outs, "out_f32 off by 8 bytes")
    _refused(call(p16=o16.ptr + 4), "layernorm", outs, "out16 off by 4 bytes")


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_cast_f32_16

def _f32_from_bits(b):
    return torch.tensor([b], dtype=torch.int64).to(torch.int32).view(F32).item() if b < 2 ** 31 else \
        torch.tensor([b - 2 ** 32], dtype=torch.int64).to(torch.int32).view(F32).item()


def _cast_planted(dt):
    """fp32 values at the edges of the rounding into dt"""
    inf, nan = float("inf"), float("nan")
    if dt == F16:
        u = 2.0 ** -11
        v = [1 + u, 1 + 3 * u, -(1 + u), -(1 + 3 * u),                           # exact ties: to even, down and up
             1 + u + 2.0 ** -23, 1 + u - 2.0 ** -23,                               # one fp32 ulp beside a tie
             65504.0, 65519.99609375, 65520.0, -65520.0, 65536.0,                  # the largest finite value; the first that rounds to inf
             2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23), 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 2.0 ** -14 - 2.0 ** -25,  # subnormals, ties among them
             1e-10, -1e-10, 2.0 ** -26]                                            # round to 0
    else:
        u = 2.0 ** -8
        v = [1 + u, 1 + 3 * u, -(1 + u), -(1 + 3 * u), 1 + u + 2.0 ** -23, 1 + u - 2.0 ** -23,
             _f32_from_bits(0x7F7F0000), _f32_from_bits(0x7F7F7FFF), _f32_from_bits(0x7F7F8000), -_f32_from_bits(0x7F7F8000),
             _f32_from_bits(0x7F7FFFFF),                                           # max bf16; below / at the tie to inf; max fp32
             2.0 ** -126, 2.0 ** -126 * (1 + 2.0 ** -8), 2.0 ** -126 * (1 + 3 * 2.0 ** -8)]
    return torch.tensor(v + [0.0, -0.0, inf, -inf, nan], dtype=F64).float()


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("n", CAST_N)
def test_cast_f32_16(gpu, n, dt):
    dev = gpu["device"]
    g_ = _gen(4000 + n)
    x = torch.randn(n, generator=g_) * torch.ldexp(torch.ones(n), torch.randint(-18, 15, (n,), generator=g_))
    pl = _cast_planted(dt)
    k = pl.numel()
    if n >= 2 * k:          # at the head, and reversed at the end: the ties lie in the tail (n % 8 elements)
        x[:k], x[n - k:] = pl, pl.flip(0)
    else:                   # all planted
        x = pl.roll(n)[:n].clone() if n < k else torch.cat([pl, pl.flip(0)])[:n].clone()
    pad = 64
    X = torch.full((n + 2 * pad,), float("nan"), dtype=F32)
    X[pad:pad + n] = x
    X = X.to(dev)
    X0 = X.clone()
    want = x.to(dt)         # the CPU's round-to-nearest-even conversion
    what = f"cast_f32_16 n={n} {_name(dt)}"
    outs = []
    for _ in range(2):
        out = torch.full((n + 2 * pad,), float("nan"), dtype=dt, device=dev)
        out0 = out.clone()
        _ok(_L().tcavt_cast_f32_16(X[pad:].data_ptr(), out[pad:].data_ptr(), n, _dt_code(dt), _st()), what)
        assert _same_bits(out[:pad], out0[:pad]) and _same_bits(out[pad + n:], out0[pad + n:]), what + ": write outside the range"
        assert _same_bits(X, X0), what + ": input modified"
        outs.append(out[pad:pad + n].cpu())
    got = outs[0]
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what + ": NaN does not stay NaN (or appears)"
    bad = (_bits(got) != _bits(want)) & ~nan
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} elements differ; first {_first_bad(bad)}: x {x[_first_bad(bad)].item()!r} "
                                 f"got {got[_first_bad(bad)].item()!r} want {want[_first_bad(bad)].item()!r}")
    assert _same_bits(outs[1], got), what + ": not reproducible"


def test_cast_refusals(gpu):
    dev = gpu["device"]
    x = torch.randn(64, device=dev)
    o = _guarded(1, 64, BF16, dev)
    L = _L()
    _refused(L.tcavt_cast_f32_16(x.data_ptr(), o.ptr, 0, _dt_code(BF16), _st()), "cast", [o], "n = 0")
    _refused(L.tcavt_cast_f32_16(x.data_ptr(), o.ptr, 64, _dt_code(F32), _st()), "cast", [o], "dtype16 = TCAVT_F32")
    _refused(L.tcavt_cast_f32_16(x.data_ptr() + 4, o.ptr, 32, _dt_code(BF16), _st()), "cast", [o], "x off by 4 bytes")
    _refused(L.tcavt_cast_f32_16(x.data_ptr(), o.ptr + 2, 32, _dt_code(BF16), _st()), "cast", [o], "out off by 2 bytes")


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_embed_fuse, tcavt_rownorm_prep

def _sumsq_bound(ref, terms):
    """part[:, 0]: the row's sum of squares; every square rounds, a lane adds `terms` of them, six exchange levels: n = terms + 6 + 1
    relative on a sum of non-negative terms; fp32 output"""
    return 1.01 * (terms + 6 + 1) * _E * ref + _ulp(ref, F32)


class Embed:
    """the operands of one tcavt_embed_fuse case on the device, and h as ONE fp32 addition in torch on the CPU"""

    def __init__(self, case, tdt, dev, seed, ids=None):
        B, Nq, Lt, H, V = case
        g_ = _gen(seed)
        self.case, self.tdt, self.dev = case, tdt, dev
        self.table = Poisoned(V, H, tdt, dev, ld=H, extra_rows=3, fill=torch.randn(V, H, generator=g_))
        if ids is None:
            ids = torch.randint(0, V, (B, max(Lt, 1)), generator=g_)
            ids.view(-1)[0], ids.view(-1)[-1] = V - 1, 0
        self.ids = ids.to(dev)
        self.img = Poisoned(B * max(Nq, 1), H, F32, dev, ld=H, extra_rows=3, fill=torch.randn(B * max(Nq, 1), H, generator=g_))
        self.vis, self.txt = (torch.randn(H, generator=g_) * 0.5).to(dev), (torch.randn(H, generator=g_) * 0.5).to(dev)
        self.ins = [("table", self.table.buf, self.table.before), ("img", self.img.buf, self.img.before),
                    ("ids", self.ids.view(torch.int32), self.ids.view(torch.int32).clone()), ("vis_mod", self.vis, self.vis.clone()), ("txt_mod", self.txt, self.txt.clone())]
        self.rows = B * (Nq + Lt)
        # image rows: 4 squares per 256-column step; text rows: 8 per 512-column step (per lane, serially)
        t_img, t_txt = 4 * -(-H // 256), 8 * -(-H // 512)
        self.terms = torch.tensor([t_img if i < Nq else t_txt for _ in range(B) for i in range(Nq + Lt)], dtype=F64)[:, None]

    def h_cpu(self, ids=None):
        B, Nq, Lt, H, V = self.case
        ids = self.ids.cpu() if ids is None else ids
        parts = []
        if Nq:
            parts.append(self.img.region.cpu().view(B, Nq, H) + self.vis.cpu())
        if Lt:
            parts.append(self.table.region.cpu()[ids[:, :Lt]].float() + self.txt.cpu())
        return torch.cat(parts, 1).reshape(self.rows, H)

    def call(self, h, h16, part, npart, scale, flag, table_dtype=None, H=None, table=None, img=None, vis=None, txt=None):
        B, Nq, Lt, H0, V = self.case
        return _L().tcavt_embed_fuse(table or self.table.buf.data_ptr(), self.ids.data_ptr(), img or self.img.buf.data_ptr(),
                                     vis or self.vis.data_ptr(), txt or self.txt.data_ptr(), h, B, Nq, Lt, H or H0, V, flag,
                                     _dt_code(self.tdt) if table_dtype is None else table_dtype, h16, part, npart, scale, _st())


def _flag(dev):
    f = torch.tensor([0x55555555, 0, 0x2AAAAAAA, 0], dtype=torch.int32, device=dev)
    return f, f[1:].data_ptr()


def _embed_call_checked(e, with_h, with16, scale, npart, what, key):
    """one call into fresh guarded outputs, everything checked; returns (h, h16, part) Guarded or None"""
    H, dev, tdt = e.case[3], e.dev, e.tdt
    h = _guarded(e.rows, H, F32, dev) if with_h else None
    h16 = _guarded(e.rows, H, tdt, dev) if with16 else None
    part = _guarded(e.rows, npart, F32, dev) if with16 else None
    flag, fp = _flag(dev)
    _ok(e.call(h.ptr if h else None, h16.ptr if h16 else None, part.ptr if part else None, npart, scale, fp), what)
    for o in (h, h16, part):
        if o:
            o.check(what)
    _unchanged(e.ins, what)
    assert flag.tolist() == [0x55555555, 0, 0x2AAAAAAA, 0], what + ": a clean call touched the flag (or its neighbours)"
    want = e.h_cpu()
    s = 1.0 if scale == 0 else scale
    if with_h:
        _bits_equal(h.region, want, what + ": h is not the fp32 sum")
    if with16:
        want16 = (want * s).to(tdt)
        _bits_equal(h16.region, want16, what + ": h16 != round(scale * h)")
        summed = (want * s).double() if with_h else want16.double()     # the unrounded scaled values / the stream's own content
        ref = (summed * summed).sum(1, keepdim=True)
        _check(part.region[:, :1], ref, _sumsq_bound(ref, e.terms), what + " part[:, 0]", key)
        assert bool((part.region[:, 1:] == 0).all()), what + ": part[:, 1:] is not exactly 0"
    return h, h16, part


@pytest.mark.parametrize("tdt", DTYPES, ids=_name)
@pytest.mark.parametrize("case", EMBED_CASES, ids=lambda c: "x".join(map(str, c)))
def test_embed_fuse(gpu, case, tdt):
    e = Embed(case, tdt, gpu["device"], 5000 + case[3])
    for with_h, with16, scale, n in EMBED_CALLS:
        npart = _npart(n, case[3])
        what = f"embed_fuse {case} {_name(tdt)} h={with_h} h16={with16} scale={scale} npart={npart}"
        key = ("tcavt_embed_fuse", "embed_fuse_kernel part" + ("" if with_h else " (h == NULL: rounded values)"), _name(tdt))
        a = _embed_call_checked(e, with_h, with16, scale, npart, what, key)
        b = _embed_call_checked(e, with_h, with16, scale, npart, what + " again", key)
        for x, y in zip(a, b):
            assert x is None or _same_bits(x.region, y.region), what + ": not reproducible"


@pytest.mark.parametrize("tdt", DTYPES, ids=_name)
def test_embed_fuse_bad_ids(gpu, tdt):
    """ids -1, V and 2^40 each set the flag and yield row 0 of the table; the other rows are as in the clean call"""
    dev = gpu["device"]
    case = (3, 4, 9, 256, 50)
    B, Nq, Lt, H, V = case
    clean = torch.randint(1, V, (B, Lt), generator=_gen(77))
    for bad, where in ((-1, (0, 0)), (V, (1, 4)), (2 ** 40, (2, 8))):
        ids = clean.clone()
        ids[where] = bad
        e = Embed(case, tdt, dev, 5100, ids=ids)
        h = _guarded(e.rows, H, F32, dev)
        flag, fp = _flag(dev)
        what = f"embed_fuse bad id {bad}"
        _ok(e.call(h.ptr, None, None, 0, 0.0, fp), what)
        h.check(what)
        _unchanged(e.ins, what)
        assert flag.tolist() == [0x55555555, 1, 0x2AAAAAAA, 0], f"{what}: flag {flag.tolist()}"
        as_zero = ids.clone()
        as_zero[where] = 0
        _bits_equal(h.region, e.h_cpu(as_zero), what + ": the row of a bad id is not row 0 of the table (+ txt_mod)")


def test_embed_fuse_refusals(gpu):
    """read from embed_fuse_impl: h16 and part go together, 0 <= stream_scale <= 1, H % 8, the table type, an output, the
    alignment of what the kernel reads and writes with 8- and 16-byte accesses -- all before the launch"""
    dev = gpu["device"]
    e = Embed((2, 2, 3, 64, 9), F16, dev, 5200)
    h, h16, part = _guarded(e.rows, 64, F32, dev), _guarded(e.rows, 64, F16, dev), _guarded(e.rows, 4, F32, dev)
    outs = [h, h16, part]
    flag, fp = _flag(dev)
    _refused(e.call(h.ptr, h16.ptr, None, 4, 0.0, fp), "embed_fuse", outs, "h16 without part")
    _refused(e.call(h.ptr, None, part.ptr, 4, 0.0, fp), "embed_fuse", outs, "part without h16")
    _refused(e.call(h.ptr, h16.ptr, part.ptr, 0, 0.0, fp), "embed_fuse", outs, "npart = 0")
    _refused(e.call(h.ptr, h16.ptr, part.ptr, 4, 2.0, fp), "embed_fuse", outs, "stream_scale = 2")
    _refused(e.call(h.ptr, h16.ptr, part.ptr, 4, -0.5, fp), "embed_fuse", outs, "stream_scale = -0.5")
    _refused(e.call(h.ptr, None, None, 0, 0.0, fp, H=12), "embed_fuse", outs, "H = 12")
    _refused(e.call(h.ptr, None, None, 0, 0.0, fp, table_dtype=_dt_code(F32)), "embed_fuse", outs, "table_dtype = TCAVT_F32")
    _refused(e.call(h.ptr, None, None, 0, 0.0, fp, table_dtype=9), "embed_fuse", outs, "table_dtype = 9")
    _refused(e.call(None, None, None, 0, 0.0, fp), "embed_fuse", outs, "no output")
    _refused(e.call(h.ptr, None, None, 0, 0.0, None), "embed_fuse", outs, "no flag")
    _refused(e.call(h.ptr + 8, None, None, 0, 0.0, fp), "embed_fuse", outs, "h off by 8 bytes")
    _refused(e.call(h.ptr, h16.ptr + 4, part.ptr, 4, 0.0, fp), "embed_fuse", outs, "h16 off by 4 bytes")
    _refused(e.call(h.ptr, None, None, 0, 0.0, fp, table=e.table.buf.data_ptr() + 8), "embed_fuse", outs, "table off by 8 bytes")
    _refused(e.call(h.ptr, None, None, 0, 0.0, fp, img=e.img.buf.data_ptr() + 4), "embed_fuse", outs, "img off by 4 bytes")
    _refused(e.call(h.ptr, None, None, 0, 0.0, fp, vis=e.vis.data_ptr() + 4), "embed_fuse", outs, "vis_mod off by 4 bytes")
    _refused(e.call(h.ptr, None, None, 0, 0.0, fp, txt=e.txt.data_ptr() + 8), "embed_fuse", outs, "txt_mod off by 8 bytes")
    assert flag.tolist() == [0x55555555, 0, 0x2AAAAAAA, 0]


def _prep_call(X, x16, part, M, H, npart, dt, rounded, scale):
    return _L().tcavt_rownorm_prep(X, x16, part, M, H, npart, _dt_code(dt), rounded, scale, _st())


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("M,H", PREP_CASES)
def test_rownorm_prep(gpu, M, H, dt):
    dev = gpu["device"]
    g_ = _gen(6000 + H)
    x = torch.randn(M, H, generator=g_) * torch.ldexp(torch.ones(M, 1), torch.randint(-2, 3, (M, 1), generator=g_))
    X = Poisoned(M, H, F32, dev, ld=H, extra_rows=3, fill=x)
    x_cpu = X.region.cpu()
    terms = 4 * -(-(H // 4) // 64)
    for rounded, scale, npart in PREP_CALLS:
        what = f"rownorm_prep {M}x{H} {_name(dt)} rounded={rounded} scale={scale} npart={npart}"
        key = ("tcavt_rownorm_prep", "rownorm_prep_kernel" + (" rounded sums" if rounded else ""), _name(dt))
        want16 = (x_cpu * scale).to(dt)
        summed = want16.double() if rounded else (x_cpu * scale).double()
        ref = (summed * summed).sum(1, keepdim=True)
        got = []
        for tag in ("", " again"):
            x16, part = _guarded(M, H, dt, dev), _guarded(M, npart, F32, dev)
            _ok(_prep_call(X.buf.data_ptr(), x16.ptr, part.ptr, M, H, npart, dt, rounded, scale), what + tag)
            x16.check(what + tag)
            part.check(what + tag)
            _unchanged([("x", X.buf, X.before)], what + tag)
            _bits_equal(x16.region, want16, what + tag + ": x16 != round(scale * x)")
            _check(part.region[:, :1], ref, _sumsq_bound(ref, terms), what + tag + " part[:, 0]", key)
            assert bool((part.region[:, 1:] == 0).all()), what + ": part[:, 1:] is not exactly 0"
            got.append((x16, part))
        assert _same_bits(got[0][0].region, got[1][0].region) and _same_bits(got[0][1].region, got[1][1].region), what + ": not reproducible"


@pytest.mark.parametrize("tdt", DTYPES, ids=_name)
@pytest.mark.parametrize("case", [(3, 4, 9, 256, 50), (5, 3, 2, 264, 7)], ids=lambda c: "x".join(map(str, c)))
def test_rownorm_prep_equals_embed_fuse(gpu, case, tdt):
    """the h16 / part of tcavt_embed_fuse and of tcavt_rownorm_prep on the same rows h: the same bits for the 16-bit copy, the same
    float64 value inside each kernel's own bound for part (an image row adds 4 squares per lane and step in both, a text row 8 in
    embed_fuse) -- with the sums of the unrounded values (h given) and of the rounded ones (h == NULL)"""
    dev = gpu["device"]
    H = case[3]
    e = Embed(case, tdt, dev, 6100 + H)
    terms = 4 * -(-(H // 4) // 64)
    for with_h, rounded in ((1, 0), (0, 1)):
        what = f"embed_fuse / rownorm_prep {case} {_name(tdt)} rounded={rounded}"
        key = ("tcavt_embed_fuse", "embed_fuse_kernel part" + ("" if with_h else " (h == NULL: rounded values)"), _name(tdt))
        _, h16, part = _embed_call_checked(e, with_h, 1, 0.25, 4, what, key)
        h = torch.full((e.rows + 3, H), float("nan"), device=dev)
        h[:e.rows] = e.h_cpu().to(dev)
        x16, part2 = _guarded(e.rows, H, tdt, dev), _guarded(e.rows, 4, F32, dev)
        _ok(_prep_call(h.data_ptr(), x16.ptr, part2.ptr, e.rows, H, 4, tdt, rounded, 0.25), what)
        assert _same_bits(x16.region, h16.region), what + ": the 16-bit copies differ"
        summed = x16.region.double().cpu() if rounded else (e.h_cpu() * 0.25).double()
        ref = (summed * summed).sum(1, keepdim=True)
        _check(part2.region[:, :1], ref, _sumsq_bound(ref, terms), what + " rownorm_prep part",
               ("tcavt_rownorm_prep", "rownorm_prep_kernel" + (" rounded sums" if rounded else ""), _name(tdt)))
        _check(part.region[:, :1], ref, _sumsq_bound(ref, e.terms), what + " embed_fuse part", key)


def test_rownorm_prep_refusals(gpu):
    dev = gpu["device"]
    x = torch.randn(2, 64, device=dev)
    x16, part = _guarded(2, 64, F16, dev), _guarded(2, 4, F32, dev)
    outs = [x16, part]
    _refused(_prep_call(x.data_ptr(), x16.ptr, part.ptr, 2, 6, 4, F16, 0, 1.0), "rownorm_prep", outs, "H = 6")
    _refused(_prep_call(x.data_ptr(), x16.ptr, part.ptr, 2, 64, 0, F16, 0, 1.0), "rownorm_prep", outs, "npart = 0")
    _refused(_prep_call(x.data_ptr(), x16.ptr, part.ptr, 2, 64, 4, F32, 0, 1.0), "rownorm_prep", outs, "dtype16 = TCAVT_F32")
    _refused(_prep_call(x.data_ptr(), x16.ptr, part.ptr, 2, 64, 4, F16, 0, 2.0), "rownorm_prep", outs, "stream_scale = 2")
    _refused(_prep_call(x.data_ptr(), x16.ptr, None, 2, 64, 4, F16, 0, 1.0), "rownorm_prep", outs, "part NULL")
    _refused(_prep_call(x.data_ptr() + 4, x16.ptr, part.ptr, 2, 32, 4, F16, 0, 1.0), "rownorm_prep", outs, "x off by 4 bytes")
    _refused(_prep_call(x.data_ptr(), x16.ptr + 8, part.ptr, 2, 32, 4, F16, 0, 1.0), "rownorm_prep", outs, "x16 off by 8 bytes")


def test_report_worst_ratio(gpu):
    """(runs last in file order) prints the worst fraction of the bound measured in this session per (entry, instantiation, type)"""
    for k in sorted(_WORST):
        print(f"{k[0]:20s} {k[2]:5s} {k[3] if len(k) > 3 else 'f32':4s} {k[1]:60s} worst frac {_WORST[k]:7.3f}")
