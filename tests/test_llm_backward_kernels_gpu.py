"""The row, SiLU and LoRA-gradient kernels of the decoder backward (csrc/llm_backward.hip, csrc/stack.hip) against float64.

Every case calls the C entry point (capi.lib().tcavt_*) and checks every element against ONE float64 evaluation of the operation in
torch, from the same 16-bit / fp32 input values.  Nothing in a reference comes from a project kernel: dropout masks are
oracle/philox.py keep_mask(M * H, p, seed, site) with element index m * H + k, 1 / (1 - p) is the host's fp32 quotient,
rs[m] = 1 / sqrt(sum(part[m]) / H + eps) from the fp32 `part` the test passes in, and the power-of-two scale handed to
tcavt_rmsnorm_bwd is first compared with the host's own evaluation of the rule.

Buffers: every output lies in a larger NaN-filled allocation with guard rows before and after and a padded leading dimension
wherever the entry point takes one (ldg, ldx, ldc); every in-range element must come back finite and inside its bound, every guard
element keep its bits, every input stay bit-unchanged.  Each case runs in fp16 and bf16 where the kernel has both forms.

Two regimes:

- exact (bit for bit; wherever no rsqrt enters: tcavt_wgrad_tn without rs_part, tcavt_lora_down, tcavt_lora_dgrad).  Operands are
  small integers, dropout runs at p = 0.5 (1 / (1 - p) = 2), so every fp32 partial sum is an integer below 2^24 in any order
  (asserted on |G|^T |X|): float atomics cannot blur the result and a wrong index, mask, site, row guard or lost token changes it.
- realistic (per-element bound).  N(0, 1)-like data with row gains.  The bound is derived next to each reference:
      |got - ref| <= c * u * unit + 1.01 * [fp32 terms] + [fp16 subnormal term] + ulp_out(ref)
  c counts the 16-bit roundings on the element's path (u = 2^-11 / 2^-8), `unit` is the product of absolute values the rounding
  acts on, the fp32 accumulation term is n * 2^-24 * unit with n = the number of terms on the longest summation chain, taken
  from the host rule (tokens per workgroup + workgroups + 1 for the weight gradients).  Where the path holds a 16-bit rounding
  the global bar per output block is rel_err(got, ref) <= 2 * rel_err(emul, ref), emul = the float64 formula with exactly those
  roundings applied (paths without one have emul == ref: the per-element fp32 bound alone judges them).

Cases (test_cases_cover_the_host_rules asserts from these lists that every instantiation and every edge is reached):

| tcavt_silu_mul_bwd (M, I) | why |
|---|---|
| (1, 16) | one thread |
| (5, 48) | 15 threads of a 256-thread block |
| (37, 128) | the earlier test's shape |
| (300, 1152) | several blocks, the last one partial |
One row holds planted gate values 0, -0.0, +-20, +-60, +-max of the type: __expf(-g) saturates, sg * (1 + g * (1 - sg)) must stay
finite and inside the bound.  In-place use (g_gu == gu) gives the bits of the out-of-place call.

| tcavt_rmsnorm_bwd (M, H) | why |
|---|---|
| (1, 8) | one lane |
| (5, 256) | M % 4 != 0: the wave-per-row guard |
| (37, 384) | the earlier test's shape |
| (4, 512) | one full step of 512 columns |
| (3, 520) | a second step for one lane |
| (6, 1032) | partial steps |
| (9, 2048), (2, 4352) | product widths: 4 and 9 steps |
24 cases walk the 8 shapes and the 12 instantiations (x fp32 / fp16 / bf16, gy fp16 / bf16, 16-bit copy fp16 / bf16) together with
the modes gy2 none / given, accumulate 0 / 1 onto a random base, gx_bf16 none / given, gy_scale none / the power of two that
tcavt_grad_scale_pick picks on the same gradients.  Row 1 is built to cancel (x = g, true gx ~ eps r^3 x), row 2 has x = 0.  The
bound carries the cancellation term |r g| + |x k|, not |gx|.  The 16-bit copy equals the fp32 output rounded once, bit for bit.
test_rmsnorm_formula_matches_autograd ties the closed form to float64 autograd (1e-12 relative).

| tcavt_wgrad_tn (M, H, n, g_col0) | why |
|---|---|
| (1, 8, 16, 0) | smallest |
| (31, 248, 32, 16) | one partial token step, partial column block |
| (33, 264, 48, 8) | a second workgroup of one token, a second column block of 8 columns |
| (1000, 712, 64, 0) | the earlier test's shape |
| (8200, 64, 32, 0) | m_per_wg = 64: two steps per workgroup, the last workgroup partial |
(G bf16, X bf16), (G bf16, X fp16), (G fp16, X fp16); trans_out 0 / 1; accumulation into a non-zero C; ldg 72 / 136 with NaN in
every column of G outside [g_col0, g_col0 + n); ldx = H + 24; ldc padded; rs_part none / given (rs_npart 4 and 32).  Exact regime
without rs_part, realistic with and without it.

| tcavt_lora_wgrad_a (M, H) | why |
|---|---|
| (1, 16) | smallest |
| (33, 240) | partial column block |
| (200, 272) | second column block of 16 columns |
| (200, 512) | the earlier test's shape |
| (8200, 256) | two steps per workgroup |
npart 4 and 8; p 0, 0.1, 0.5; site_q / site_v 77 / 1031 (site_q + 1 is wrong); gamma with a per-column pattern that is never 1;
g_t with its own gain in each of the 32 columns; dA accumulated onto a random base, rows 32..63 NaN.  The small-rms case (stream
rms 0.02, g_t ~ 600) is bounded per element like the others.

| tcavt_lora_down (M, H) | why |     | tcavt_lora_dgrad (M, H) | why |
|---|---|                              |---|---|
| (1, 256) | one token |               | (1, 128) | one token |
| (15, 256) | below one block |        | (17, 128) | one token into a second block |
| (16, 256) | exactly one block |      | (100, 384) | third wave's second round absent |
| (17, 512) | one token into a 2nd |   | (33, 2048) | a product width |
| (100, 2048) | a product width |
p 0, 0.1, 0.5 (exact regime: 0 and 0.5).  lora_down: columns 32..63 of t keep their bits.  lora_dgrad: elements dropped under both
masks are exact zeros.  Rows >= M (what a partial 16-token block clamps to) are guard rows: nothing is written there.

tcavt_grad_scale_pick (fp16 and bf16): amax a power of two, exactly target, one ulp above / below, the maximum in g_b, n = 8,
n = 8 * (1024 * 256 + 3) with the maximum in the last octet (grid-stride loop), all zero, an inf, a NaN beside finite values,
amax = 2^-125 (bf16: target / amax leaves fp32), backoff 0 / 4 / 24.  tcavt_clip_grad_norm: n 1, 1000, 1025, 300 001, grad_scale
1 and 1/4, norm below and above max_norm, all zero.

MEASURED on an MI355X: the worst fraction of the whole bound per (entry point, instantiation, type) stands beside the constants
below; every instantiation and case is in profiles/llm_backward_bounds.txt, test_report_worst_ratio prints the session's (pytest -s).
"""
import functools
import math

import numpy as np
import pytest
import torch

from test_attention_bwd_gpu import _first_bad, _last_error, _name, _rnd, _same_bits
from test_gemm_forms_gpu import Poisoned, _bits, _dt_code, _round, _ulp

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
DTYPES = [F16, BF16]
_U = {F16: 2.0 ** -11, BF16: 2.0 ** -8, F32: 0.0}  # unit roundoff of one rounding to the 16-bit type
_E = 2.0 ** -24                                    # unit roundoff of fp32
_T = 4 * _E                                        # rsqrtf / __expf / rcp: 2 ulps of the result (as the attention modules)
_R = 2.0                                           # global bar: rel_err(got, ref) <= _R * rel_err(emul, ref)
_GUARD = 3                                         # NaN rows before and after every output
EPS = float(np.float32(1e-5))                      # (the entry points take eps as a C float)
SEED, SITE_Q, SITE_V = 0xABCDE12345, 77, 1031
# MEASURED on an MI355X: worst fraction of the whole bound (bar 1.0) / worst global ratio r (bar _R = 2.0) over the cases, fp16 | bf16
# (profiles/llm_backward_bounds.txt has every instantiation).  0.5 = the output rounding alone (half of the output ulp the bound
# allows); a fraction far below it: an fp32 output whose bound is the worst-case summation chain.
#   tcavt_silu_mul_bwd                                   0.500 / 1.000 | 0.500 / 1.000
#   tcavt_rmsnorm_bwd     x fp32                         0.123 | 0.162     x fp16  0.129 | 0.318     x bf16  0.118 | 0.327  (by gy type)
#   tcavt_wgrad_tn        (G bf16, X bf16)               0.053            with rs_part  0.775 / 1.000
#                         (G bf16, X fp16)               0.619 / 1.000    with rs_part  0.670 / 1.000
#                         (G fp16, X fp16)               0.058            with rs_part  0.772 / 1.002
#   tcavt_lora_wgrad_a    p = 0                          0.735 / 1.000 | 0.785 / 1.000      small rms  0.179 / 1.000 | 0.194 / 1.000
#                         p = 0.1                        0.832 / 1.001 | 0.603 / 1.000      small rms  0.189 / 1.001 | 0.195 / 1.000
#                         p = 0.5                        0.588 / 1.000 | 0.563 / 1.000
#   tcavt_lora_down       p = 0 | 0.1 | 0.5              0.482, 0.173, 0.488 / 1.000 | 0.496, 0.183, 0.498 / 1.000
#   tcavt_lora_dgrad      every p                        0.498 / 1.000 | 0.500 / 1.000
#   tcavt_clip_grad_norm  scratch[1024], scratch[1025]   0.063
# Mutants: g * rs rounded through bf16 in wgrad_tn_kernel<fp16, fp16> gives a fraction above 1 in every case; the mutants of the
# issue (v masks from q's site, gamma dropped from column 256 on, one token lost in the last workgroup, the second 512-column
# step left out of the reduction, sg for 1 - sg, the odd quarter-wave's features moved by four) each fail their kernel's cases.
_WORST = {}   # (entry, instantiation, type) -> dict(frac=..., r=...)


def _L():
    from tcavt_amd import capi

    return capi.lib()


def _st():
    from tcavt_amd import capi

    return capi.stream_ptr()


def _ok(rc, what):
    torch.cuda.synchronize()
    assert rc == 0, f"{what}: rc {rc}: {_last_error()}"


class Guarded:
    """A [rows, cols] region inside a NaN-filled [before + rows + after, ld] buffer (guard rows on both sides, padded leading
    dimension); .region is the view, .ptr its address, .check() asserts that nothing outside the region changed."""

    def __init__(self, rows, cols, dt, dev, ld=None, fill=None, before=_GUARD, after=_GUARD):
        self.ld = cols if ld is None else ld
        assert self.ld >= cols and (before * self.ld * torch.finfo(dt).bits // 8) % 16 == 0
        self.buf = torch.full((before + rows + after, self.ld), float("nan"), dtype=dt, device=dev)
        self.rows, self.cols, self.b = rows, cols, before
        if fill is not None:
            self.region.copy_(fill.to(dt))
        self.before = self.buf.clone()

    @property
    def region(self):
        return self.buf[self.b: self.b + self.rows, : self.cols]

    @property
    def ptr(self):
        return self.region.data_ptr()

    def check(self, what):
        out = torch.ones_like(self.buf, dtype=torch.bool)
        out[self.b: self.b + self.rows, : self.cols] = False
        assert torch.equal(_bits(self.buf)[out], _bits(self.before)[out]), f"{what}: write outside [{self.rows}, {self.cols}]"


def _unchanged(pairs, what):
    for name, now, was in pairs:
        assert _same_bits(now, was), f"{what}: input {name} modified"


def _record(key, **kw):
    w = _WORST.setdefault(key, {})
    for k, v in kw.items():
        w[k] = max(w.get(k, -1.0), v)


def _check(got, ref, unit16, rest, what, key):
    """|got - ref| <= unit16 + rest per element (unit16 = c * u * unit, rest = fp32 terms + output ulp); every element finite;
    records the worst fraction of the bound"""
    g = got.double()
    assert torch.isfinite(g).all(), f"{what}: {int((~torch.isfinite(g)).sum())} non-finite (unwritten?) elements in range"
    d = (g - ref).abs()
    bound = unit16 + rest
    frac = (d / bound.clamp_min(1e-300)).max().item()
    _record(key, frac=frac)
    print(f"frac {what}: {frac:.3f}")
    bad = d > bound
    if bool(bad.any()):
        i = _first_bad(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of bound (worst fraction {frac:.3f}); first {i}: "
                             f"got {g[i].item()!r} ref {ref[i].item()!r} allowed {bound[i].item():.3e}")


def _global(got, ref, emul, what, key):
    """rel_err(got, ref) <= _R * rel_err(emul, ref) on one output block; skipped where the path has no 16-bit rounding (emul == ref)"""
    n = ref.norm().item()
    if n == 0:
        return
    eg, ee = ((got.double() - ref).norm() / n).item(), ((emul - ref).norm() / n).item()
    if ee == 0:
        return
    _record(key, r=eg / ee)
    print(f"r {what}: {eg / ee:.3f}  (rel {eg:.3e}, emulation floor {ee:.3e})")
    assert eg <= _R * ee, f"{what}: rel {eg:.3e} > {_R} * emulation floor {ee:.3e}"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, g, dev):
    return torch.randn(shape, generator=g).double().to(dev)


def _gains(n, g, dev):
    """row gains 2^-2 .. 2^2"""
    return torch.ldexp(torch.ones(n), torch.randint(-2, 3, (n,), generator=g)).double().to(dev)[:, None]


def _ints(shape, r, g, dev):
    return torch.randint(-r, r + 1, shape, generator=g).double().to(dev)


@functools.lru_cache(maxsize=None)
def _keep_np(n, p, site):
    from oracle.philox import keep_mask

    return keep_mask(n, p, SEED, site)


def _keep(M, H, p, site, dev):
    """float64 keep mask [M, H] of the Philox oracle, element index m * H + k (all ones for p = 0)"""
    if p == 0:
        return torch.ones(M, H, dtype=F64, device=dev)
    return torch.from_numpy(_keep_np(M * H, p, site).astype(np.float64)).view(M, H).to(dev)


def _inv_keep(p):
    """1 / (1 - p) as the host computes it (make_dropout: an fp32 quotient), as float64"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def _rs64(part, H):
    return 1.0 / torch.sqrt(part.double().sum(1) / H + EPS)


def _e_rs(npart):
    """relative fp32 error of part_rscale: npart additions, * inv_h (itself rounded), + eps (half of all that under the root), rsqrtf"""
    return 0.5 * (npart + 3) * _E + _T


def _split_rule(M, H):
    """(gx, workgroups along the tokens, tokens per workgroup) of tcavt_wgrad_tn / tcavt_lora_wgrad_a"""
    gx = -(-H // 256)
    split = max(1, 256 // gx)
    m_per_wg = -(-(-(-M // split)) // 32) * 32
    return gx, -(-M // m_per_wg), m_per_wg


def _n_acc(M, H):
    """terms on the longest fp32 summation chain of an element of a split weight gradient: the tokens of a workgroup (MFMA steps
    of 32, chained), one atomic per workgroup, the value already in C"""
    _, split, m_per_wg = _split_rule(M, H)
    return m_per_wg + split + 1


# ---------------------------------------------------------------------------------------------------------------------------
# case lists

SILU_CASES = [(1, 16), (5, 48), (37, 128), (300, 1152)]
RMS_SHAPES = [(1, 8), (5, 256), (37, 384), (4, 512), (3, 520), (6, 1032), (9, 2048), (2, 4352)]
RMS_INSTS = [(x, g, o) for x in (F32, F16, BF16) for g in (F16, BF16) for o in (F16, BF16)]


def _rms_case(j):
    """(M, H, x type, gy type, copy type, gy2, accumulate, copy, gy_scale)"""
    (M, H), (xdt, gdt, odt) = RMS_SHAPES[j % 8], RMS_INSTS[j % 12]
    return M, H, xdt, gdt, odt, j % 2 == 1, (j // 2) % 2 == 1, j % 5 != 0, j % 3 != 1


RMS_CASES = [_rms_case(j) for j in range(24)]
WGRAD_CASES = [(1, 8, 16, 0), (31, 248, 32, 16), (33, 264, 48, 8), (1000, 712, 64, 0), (8200, 64, 32, 0)]
WGRAD_INSTS = [(BF16, BF16), (BF16, F16), (F16, F16)]                    # (G, X)
WGRAD_LDG = [72, 136, 72, 136, 72]
WGRAD_REAL_CALLS = [(0, 0), (1, 4), (0, 32), (1, 0)]                     # (trans_out, rs_npart; 0 = no rs_part)
LORA_A_CASES = [(1, 16), (33, 240), (200, 272), (200, 512), (8200, 256)]
LORA_A_CALLS = [(0.0, 4), (0.1, 8), (0.5, 4), (0.1, 4), (0.5, 8)]        # (p, npart): call i of case i, and call i + 1
LORA_DOWN_CASES = [(1, 256), (15, 256), (16, 256), (17, 512), (100, 2048)]
LORA_DGRAD_CASES = [(1, 128), (17, 128), (100, 384), (33, 2048)]
P_VALUES = [0.0, 0.1, 0.5]
TARGET = 256.0
CLIP_N = [1, 1000, 1025, 300_001]


def _ulp_of(v, dt):
    return _ulp(torch.tensor([float(v)], dtype=F64), dt).item()


def _scale_cases(dt):
    """(name, amax, holder of the maximum, n, backoff, filler amplitude relative to amax)"""
    up = TARGET + _ulp_of(TARGET, dt)
    dn = TARGET - _ulp_of(TARGET / 2, dt)
    cs = [("pow2", 2.0 ** -3, "a", 4096, 0, 0.9), ("pow2 high", 2.0 ** 9, "a", 4096, 4, 0.9), ("not pow2", 96.0, "a", 4096, 24, 0.9),
          ("target", TARGET, "a", 4096, 0, 0.5), ("target + ulp", up, "a", 4096, 0, 0.5), ("target - ulp", dn, "a", 4096, 4, 0.5),
          ("max in g_b", 3.0, "b", 4096, 0, 0.9), ("n = 8", 0.375, "a", 8, 0, 0.5),
          ("grid stride", 3.0, "a", 8 * (1024 * 256 + 3), 0, 0.3), ("grid stride in g_b", 5.0, "b", 8 * (1024 * 256 + 3), 24, 0.3)]
    if dt == BF16:
        cs += [("quotient overflows", 2.0 ** -125, "a", 4096, 0, 0.0), ("quotient overflows, backoff", 2.0 ** -125, "a", 4096, 24, 0.0)]
    else:
        cs += [("smallest fp16", 2.0 ** -24, "a", 4096, 0, 0.0)]
    return cs


def _expected_scale(amax, target, backoff):
    """the rule of grad_scale_set_kernel on the host: S = 2^(e - 1 - backoff), target / amax = f * 2^e with f in [0.5, 1), the
    exponent clamped to +-60; S = 1 for amax = 0 or inf"""
    if amax == 0 or not math.isfinite(amax):
        return 1.0
    _, e = math.frexp(target / amax)
    return 2.0 ** max(-60, min(60, e - 1 - backoff))


def test_cases_cover_the_host_rules():
    """from the case lists alone (the host arithmetic of the entry points mirrored): every instantiation and every edge is reached"""
    # silu_mul_bwd: one thread per 16 features, 256-thread blocks
    thr = [M * (I // 16) for M, I in SILU_CASES]
    assert thr[0] == 1 and thr[1] == 15 and (37, 128) in SILU_CASES and any(t > 512 and t % 256 for t in thr)
    assert all(I % 16 == 0 and I // 16 >= 1 for _, I in SILU_CASES)
    # rmsnorm_bwd: one wave per row, four rows per block, 512 columns per step and wave
    assert {c[2:5] for c in RMS_CASES} == set(RMS_INSTS) and len(RMS_INSTS) == 12
    assert {c[:2] for c in RMS_CASES} == set(RMS_SHAPES)
    steps = {(M, H): -(-H // 512) for M, H in RMS_SHAPES}
    assert set(steps.values()) >= {1, 2, 3, 4, 9} and steps[(4, 512)] == 1 and steps[(3, 520)] == 2 and (520 - 512) // 8 == 1
    assert (1, 8) in steps and any(M % 4 for M, _ in RMS_SHAPES) and all(H % 8 == 0 for _, H in RMS_SHAPES)
    assert any(H % 512 and H > 512 for _, H in RMS_SHAPES)
    modes = {c[5:] for c in RMS_CASES}
    assert {m[0] for m in modes} == {m[1] for m in modes} == {m[2] for m in modes} == {m[3] for m in modes} == {False, True}
    assert any(m[0] and m[3] for m in modes) and any(m[1] and m[2] for m in modes)          # gy2 with gy_scale; accumulate with the copy
    assert any(c[2] == BF16 for c in RMS_CASES) and any(c[3] == F16 for c in RMS_CASES)
    for dt in (F32, F16, BF16):   # every x type with and without the scale, with and without accumulate
        assert {c[6] for c in RMS_CASES if c[2] == dt} == {c[8] for c in RMS_CASES if c[2] == dt} == {False, True}
    # wgrad_tn
    assert [_split_rule(M, H) for M, H, _, _ in WGRAD_CASES] == [(1, 1, 32), (1, 1, 32), (2, 2, 32), (3, 32, 32), (1, 129, 64)]
    assert 8200 - 128 * 64 == 8 and 1000 - 31 * 32 == 8 and 33 - 32 == 1      # the last workgroup is partial in each split case
    assert {n for _, _, n, _ in WGRAD_CASES} == {16, 32, 48, 64} and {g0 for _, _, _, g0 in WGRAD_CASES} == {0, 8, 16}
    assert 264 - 256 == 8 and 248 < 256 and 712 % 256 == 200
    assert all(g0 + n <= ldg and ldg % 8 == 0 for (_, _, n, g0), ldg in zip(WGRAD_CASES, WGRAD_LDG)) and set(WGRAD_LDG) == {72, 136}
    assert {t for t, _ in WGRAD_REAL_CALLS} == {0, 1} and {r for _, r in WGRAD_REAL_CALLS} == {0, 4, 32}
    assert set(WGRAD_INSTS) == {(BF16, BF16), (BF16, F16), (F16, F16)}
    # lora_wgrad_a (the same split rule)
    assert [_split_rule(M, H) for M, H in LORA_A_CASES] == [(1, 1, 32), (1, 2, 32), (2, 7, 32), (2, 7, 32), (1, 129, 64)]
    assert 272 - 256 == 16 and 240 < 256 and all(H % 16 == 0 for _, H in LORA_A_CASES)
    calls = {LORA_A_CALLS[(i + d) % 5] for i in range(5) for d in (0, 1)}
    assert {p for p, _ in calls} == set(P_VALUES) and {n for _, n in calls} == {4, 8}
    assert all(H % (8 * n) == 0 or H % n == 0 for _, H in LORA_A_CASES for n in (4, 8))
    assert SITE_V != SITE_Q + 1 and SITE_V != SITE_Q
    # lora_down: 16 tokens per workgroup, H / 4 columns per wave in steps of 64; lora_dgrad: waves walk the features in 128s
    assert [(-(-M // 16), M % 16) for M, _ in LORA_DOWN_CASES] == [(1, 1), (1, 15), (1, 0), (2, 1), (7, 4)]
    assert all(H % 256 == 0 for _, H in LORA_DOWN_CASES) and {H // 256 for _, H in LORA_DOWN_CASES} == {1, 2, 8}
    assert [(-(-M // 16), M % 16) for M, _ in LORA_DGRAD_CASES] == [(1, 1), (2, 1), (7, 4), (3, 1)]
    assert all(H % 128 == 0 for _, H in LORA_DGRAD_CASES) and {H // 128 for _, H in LORA_DGRAD_CASES} == {1, 3, 16}
    # grad_scale_pick: at most 1024 blocks of 256 threads, one octet per thread and round
    for dt in DTYPES:
        cs = _scale_cases(dt)
        assert any(n == 8 for _, _, _, n, _, _ in cs) and any(n // 8 > 1024 * 256 and (n // 8) % (1024 * 256) == 3 for _, _, _, n, _, _ in cs)
        assert {b for _, _, _, _, b, _ in cs} == {0, 4, 24} and {h for _, _, h, _, _, _ in cs} == {"a", "b"}
        assert any(math.frexp(a)[0] == 0.5 for _, a, *_ in cs) and any(a == TARGET for _, a, *_ in cs)
        assert any(0 < a - TARGET <= _ulp_of(TARGET, dt) for _, a, *_ in cs) and any(0 < TARGET - a <= _ulp_of(TARGET, dt) for _, a, *_ in cs)
        for _, a, *_ in cs:
            assert _rnd(torch.tensor([a], dtype=F64), dt).item() == a   # representable
    assert any(TARGET / a > 3.4e38 for _, a, *_ in _scale_cases(BF16))
    assert _expected_scale(TARGET, TARGET, 0) == 1.0 and _expected_scale(2.0 ** -125, TARGET, 0) == 2.0 ** 60
    assert _expected_scale(2.0 ** -125, TARGET, 24) == 2.0 ** 60 and _expected_scale(3.0, TARGET, 4) == 4.0
    # clip_grad_norm: 1024 partial blocks
    assert CLIP_N[0] == 1 and any(n < 1024 for n in CLIP_N[1:]) and 1025 in CLIP_N and any(n > 256 * 1024 for n in CLIP_N)


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_silu_mul_bwd

def _interleave(gate, up):
    from tcavt_amd.layout import interleave_gate_up

    return interleave_gate_up(gate.T.contiguous(), up.T.contiguous()).T.contiguous()


def _silu_ref(g, u, d):
    """float64 dL/dgate, dL/dup of silu(gate) * up and their fp32 error bounds.

    The kernel: e = __expf(-g) (relative (|g| + 4) E =: ee: the argument's product with log2 e rounds once, the exponential is
    taken to 2 ulps), sg = rcp(1 + e): absolute error sg (1 - sg) ee + 3 E sg (the sum rounds once, rcp within 1 ulp = 2 E),
    t = g * (1 - sg): |g| (dsg + E (1 - sg)) + E |t|,  s = 1 + t: + E |s|,  then three products for dgate = d u sg s and two for
    dup = d g sg.  For g >= 18, exp(-g) < 2^-25: 1 + e rounds to 1, rcp(1) = 1, 1 - sg = 0 and the kernel returns fl(d u) and
    fl(d g); against the true values that is |d u| (E + e (1 + g)) and |d g| (E + e)."""
    sg = torch.sigmoid(g)
    one_m = torch.sigmoid(-g)
    s = 1 + g * one_m
    dgate, dup = d * u * sg * s, d * g * sg
    ga = g.abs()
    ee = (ga + 4) * _E
    dsg = sg * one_m * ee + 3 * _E * sg
    dt_ = ga * (dsg + _E * one_m) + _E * (g * one_m).abs()
    e_gate = dgate.abs() * 3 * _E + (d * u).abs() * (dsg * s.abs() + sg * (dt_ + _E * s.abs()))
    e_up = dup.abs() * 2 * _E + (d * g).abs() * dsg
    big = g >= 18
    e = torch.exp(-g)
    e_gate = torch.where(big, (d * u).abs() * (_E + e * (1 + ga)), e_gate)
    e_up = torch.where(big, (d * g).abs() * (_E + e), e_up)
    return dgate, dup, e_gate, e_up


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("M,I", SILU_CASES)
def test_silu_mul_bwd(gpu, M, I, dt):
    dev = gpu["device"]
    g_ = _gen(100 + M)
    gate = _rnd(_randn((M, I), g_, dev) * 2 * _gains(M, g_, dev), dt)
    up = _rnd(_randn((M, I), g_, dev), dt)
    d = _rnd(_randn((M, I), g_, dev) * _gains(M, g_, dev), dt)
    row = M // 2
    fmax = torch.finfo(dt).max
    planted = torch.tensor([0.0, -0.0, 20.0, -20.0, 60.0, -60.0, fmax, -fmax], dtype=F64, device=dev)
    gate[row, :8] = planted
    sign = torch.tensor([1.0, -1.0], dtype=F64, device=dev).repeat(I // 2)
    up[row], d[row] = 0.5 * sign, 0.5 * sign.roll(1).roll(I // 16)   # |d g| <= max / 2: the true values are inside the type's range
    gu = Poisoned(M, 2 * I, dt, dev, ld=2 * I, extra_rows=3, fill=_interleave(gate, up))
    ga = Poisoned(M, I, dt, dev, ld=I, extra_rows=3, fill=d)
    out = Guarded(M, 2 * I, dt, dev)
    what = f"silu_mul_bwd {M}x{I} {_name(dt)}"
    _ok(_L().tcavt_silu_mul_bwd(gu.buf.data_ptr(), ga.buf.data_ptr(), out.ptr, M, I, _dt_code(dt), _st()), what)
    out.check(what)
    _unchanged([("gu", gu.buf, gu.before), ("g_act", ga.buf, ga.before)], what)
    gv = gu.region.double().view(M, I // 16, 2, 16)
    g64, u64, d64 = gv[:, :, 0].reshape(M, I), gv[:, :, 1].reshape(M, I), ga.region.double()
    assert torch.equal(g64, gate) and torch.equal(u64, up)   # (the layout helper and the view of it agree)
    dgate, dup, e_gate, e_up = _silu_ref(g64, u64, d64)
    ref, f32 = _interleave(dgate, dup), _interleave(e_gate, e_up)
    key = ("tcavt_silu_mul_bwd", "silu_mul_bwd_kernel", _name(dt))
    _check(out.region, ref, 0 * ref, 1.01 * f32 + _ulp(ref, dt), what, key)
    rows = [r for r in range(M) if r != row]
    if rows:   # (the planted row's +-max / 2 would dominate the norm)
        _global(out.region[rows], ref[rows], _rnd(ref[rows], dt), what, key)
    # in place, as the product calls it: the same bits
    inpl = Guarded(M, 2 * I, dt, dev, fill=gu.region)
    _ok(_L().tcavt_silu_mul_bwd(inpl.ptr, ga.buf.data_ptr(), inpl.ptr, M, I, _dt_code(dt), _st()), what + " in place")
    inpl.check(what + " in place")
    assert _same_bits(inpl.region, out.region), f"{what}: in place differs from out of place"


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_rmsnorm_bwd

def _rms_ref(x, gamma, gy, gy2, S, base):
    """gx = r g - x r^3 mean(g x) (+ base) in float64, g = (gy + gy2) * gamma * S, and the fp32 error bound of the kernel.

    n = H / 64 + 14 bounds a reduction's chain (a lane adds 8 * ceil(H / 512) <= H / 64 + 8 terms, six exchange levels).
    g: one addition and one product (gamma * S is exact, S a power of two): 2 E.  r = rsqrtf(ss / H + eps): half of (n + 2) E under
    the root, plus the root itself: er.  k = dot / H * r^3: four operations and three factors r on |k|, and dot's own
    (n + 2) E * sum|g x| / H * r^3.  Each output: r * g (er + 2 E + E), x * k (E on top of k's error), one subtraction
    (E (|r g| + |x k|): the cancellation term), one more addition when accumulating."""
    H = x.shape[1]
    g = (gy + (gy2 if gy2 is not None else 0)) * gamma[None, :] * S
    r = 1 / torch.sqrt((x * x).mean(1, keepdim=True) + EPS)
    k = (g * x).mean(1, keepdim=True) * r ** 3
    rg, xk = r * g, x * k
    ref = rg - xk + (base if base is not None else 0)
    n = H / 64 + 14
    er = (0.5 * (n + 2) + 4) * _E
    ek = k.abs() * (4 * _E + 3 * er) + (n + 2) * _E * (g * x).abs().mean(1, keepdim=True) * r ** 3
    f32 = rg.abs() * (er + 4 * _E) + x.abs() * ek + 2 * _E * xk.abs()
    if base is not None:
        f32 = f32 + _E * (rg.abs() + xk.abs() + base.abs())
    return ref, f32, rg


def test_rmsnorm_formula_matches_autograd(gpu):
    dev = gpu["device"]
    g_ = _gen(7)
    x = _randn((9, 520), g_, dev).requires_grad_(True)
    gamma, gy, gy2 = _randn((520,), g_, dev) * 0.1 + 1, _randn((9, 520), g_, dev), _randn((9, 520), g_, dev)
    y = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + EPS) * gamma
    y.backward((gy + gy2) * 0.25)
    ref, _, _ = _rms_ref(x.detach(), gamma, gy, gy2, 0.25, None)
    assert ((ref - x.grad).norm() / x.grad.norm()).item() < 1e-12


def _pick_scale(a, b, dt, dev, backoff=None):
    """tcavt_grad_scale_pick into a guarded scale pair; returns (Guarded scale, scratch)"""
    scale = Guarded(1, 2, F32, dev, ld=8, before=2, after=2)
    scratch = torch.tensor([0x55555555, 0, 0x2AAAAAAA], dtype=torch.int32, device=dev)
    bo = torch.tensor([7, backoff, 9], dtype=torch.int32, device=dev) if backoff is not None else None
    n = a.numel()
    rc = _L().tcavt_grad_scale_pick(a.data_ptr(), b.data_ptr() if b is not None else None, n, _dt_code(dt), TARGET, scale.ptr,
                                    scratch[1:].data_ptr(), bo[1:].data_ptr() if bo is not None else None, _st())
    _ok(rc, "grad_scale_pick")
    scale.check("grad_scale_pick scale")
    assert scratch.tolist() == [0x55555555, 0, 0x2AAAAAAA], "grad_scale_pick: the scratch word is not back to 0 (or its neighbours moved)"
    assert bo is None or bo.tolist() == [7, backoff, 9]
    return scale


@pytest.mark.parametrize("j", range(24))
def test_rmsnorm_bwd(gpu, j):
    dev = gpu["device"]
    M, H, xdt, gdt, odt, two, acc, copy, scaled = RMS_CASES[j]
    g_ = _gen(200 + j)
    gamma = (0.5 + torch.rand(H, generator=g_)).to(dev)
    gy = _rnd(_randn((M, H), g_, dev) * _gains(M, g_, dev) * 2.0 ** -6, gdt)
    gy2 = _rnd(_randn((M, H), g_, dev) * 2.0 ** -7, gdt) if two else None
    x = _randn((M, H), g_, dev) * _gains(M, g_, dev)
    if M >= 2:   # a row built to cancel: x = g (up to x's rounding), true gx = eps r^3 x
        x[1] = (gy[1] + (gy2[1] if two else 0)) * gamma.double() * 64
    if M >= 3:   # x = 0: r = eps^-1/2 ~ 316; the gradient of this row is kept small so that the fp16 copy stays in range
        x[2] = 0
        gy[2] = gy[2] * 2.0 ** -6
        if two:
            gy2[2] = gy2[2] * 2.0 ** -6
    X = Poisoned(M, H, xdt, dev, ld=H, extra_rows=3, fill=x)
    GY = Poisoned(M, H, gdt, dev, ld=H, extra_rows=3, fill=gy)
    GY2 = Poisoned(M, H, gdt, dev, ld=H, extra_rows=3, fill=gy2) if two else None
    base = torch.randn(M, H, generator=g_).to(dev) if acc else None
    out = Guarded(M, H, F32, dev, fill=base)
    out16 = Guarded(M, H, odt, dev) if copy else None
    S, scale = 1.0, None
    if scaled:
        scale = _pick_scale(GY.buf[:M], GY2.buf[:M] if two else None, gdt, dev)
        amax = max(GY.region.double().abs().max().item(), GY2.region.double().abs().max().item() if two else 0.0)
        S = _expected_scale(amax, TARGET, 0)
        assert scale.region[0, 0].item() == S and scale.region[0, 1].item() == 1 / S and TARGET / 2 <= amax * S <= TARGET
    inst = f"rmsnorm_bwd_kernel<g {_name(gdt)}, o {_name(odt) if copy else '-'}, x {_name(xdt)}>"
    what = f"rmsnorm_bwd {M}x{H} {inst} gy2={two} acc={acc} scale={S}"
    gam0 = gamma.clone()
    rc = _L().tcavt_rmsnorm_bwd(X.buf.data_ptr(), gamma.data_ptr(), GY.buf.data_ptr(), GY2.buf.data_ptr() if two else None, EPS,
                                out.ptr, out16.ptr if copy else None, int(acc), M, H, _dt_code(gdt), _dt_code(odt),
                                scale.ptr if scaled else None, _dt_code(xdt), _st())
    _ok(rc, what)
    out.check(what)
    pairs = [("x", X.buf, X.before), ("gy", GY.buf, GY.before), ("gamma", gamma, gam0)]
    if two:
        pairs.append(("gy2", GY2.buf, GY2.before))
    _unchanged(pairs, what)
    ref, f32, rg = _rms_ref(X.region.double(), gamma.double(), GY.region.double(), GY2.region.double() if two else None, S,
                            base.double() if acc else None)
    _check(out.region, ref, 0 * ref, 1.01 * f32 + _ulp(ref, F32), what, ("tcavt_rmsnorm_bwd", inst, _name(gdt)))
    if M >= 2:   # the cancelling row really cancels: its gradient is far below its two terms
        assert (ref[1] - (base[1].double() if acc else 0)).abs().max().item() < 2.0 ** -5 * rg[1].abs().max().item()
    if copy:
        out16.check(what + " 16-bit copy")
        assert torch.isfinite(out16.region.float()).all(), what + ": 16-bit copy not finite"
        assert _same_bits(out16.region, _round(out.region, odt)), what + ": the 16-bit copy is not the fp32 output rounded once"


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_wgrad_tn

class WOperands:
    """G [M, ldg] with NaN outside columns [g0, g0 + n) and in three rows behind M; X [M, ldx = H + 24] likewise"""

    def __init__(self, M, H, n, g0, ldg, gdt, xdt, regime, seed, dev):
        g_ = _gen(seed)
        if regime == "exact":
            gv, xv = _ints((M, n), 4, g_, dev), _ints((M, H), 4, g_, dev)
        else:
            gv, xv = _randn((M, n), g_, dev) * _gains(M, g_, dev), _randn((M, H), g_, dev)
        self.G = torch.full((M + 3, ldg), float("nan"), dtype=gdt, device=dev)
        self.G[:M, g0:g0 + n] = gv.to(gdt)
        self.G0 = self.G.clone()
        self.X = Poisoned(M, H, xdt, dev, ld=H + 24, extra_rows=3, fill=xv)
        self.g64, self.x64 = self.G[:M, g0:g0 + n].double(), self.X.region.double()
        self.gen, self.ldg = g_, ldg
        # partial sums of squares for rs: row scales 1/4, 1, 4 around rs_h / npart
        self.parts = {}
        for npart in (4, 32):
            sc = torch.ldexp(torch.ones(M), 2 * torch.randint(-1, 2, (M,), generator=g_))[:, None]
            self.parts[npart] = ((0.25 + torch.rand(M, npart, generator=g_)) * (512 / npart) * sc).to(dev)

    def unchanged(self, what):
        _unchanged([("G", self.G, self.G0), ("X", self.X.buf, self.X.before)], what)


def _wgrad_call(op, case, gdt, xdt, trans, C, part, npart):
    M, H, n, g0 = case
    return _L().tcavt_wgrad_tn(op.G.data_ptr(), op.ldg, g0, n, op.X.buf.data_ptr(), op.X.ld, _dt_code(xdt), C.ptr, C.ld, M, H, trans,
                               _dt_code(gdt), part.data_ptr() if part is not None else None, npart, 512, EPS, _st())


def _c_buffer(n, H, trans, base, dev):
    """C [n, H] with ldc = H + 16, or C^T [H, n] with ldc = 72 (columns >= n are guard columns)"""
    return Guarded(H, n, F32, dev, ld=72, fill=base.T) if trans else Guarded(n, H, F32, dev, ld=H + 16, fill=base)


@pytest.mark.parametrize("gdt,xdt", WGRAD_INSTS, ids=lambda d: _name(d))
@pytest.mark.parametrize("ci", range(len(WGRAD_CASES)), ids=lambda i: "x".join(map(str, WGRAD_CASES[i])))
def test_wgrad_tn_exact(gpu, ci, gdt, xdt):
    dev = gpu["device"]
    M, H, n, g0 = WGRAD_CASES[ci]
    op = WOperands(M, H, n, g0, WGRAD_LDG[ci], gdt, xdt, "exact", 300 + ci, dev)
    base = _ints((n, H), 8, op.gen, dev)
    ref = base + op.g64.T @ op.x64
    assert (base.abs() + op.g64.abs().T @ op.x64.abs()).max().item() < 2.0 ** 24   # every partial sum is exact in any order
    for trans in (0, 1):
        what = f"wgrad_tn exact {WGRAD_CASES[ci]} G {_name(gdt)} X {_name(xdt)} trans={trans}"
        C = _c_buffer(n, H, trans, base, dev)
        _ok(_wgrad_call(op, WGRAD_CASES[ci], gdt, xdt, trans, C, None, 0), what)
        C.check(what)
        op.unchanged(what)
        got = C.region.T if trans else C.region
        bad = got.double() != ref
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ; first {_first_bad(bad)}"


@pytest.mark.parametrize("gdt,xdt", WGRAD_INSTS, ids=lambda d: _name(d))
@pytest.mark.parametrize("ci", range(len(WGRAD_CASES)), ids=lambda i: "x".join(map(str, WGRAD_CASES[i])))
def test_wgrad_tn_realistic(gpu, ci, gdt, xdt):
    """16-bit roundings on the path: an fp16 X under a bf16 G passes one bf16 rounding while it is staged (u_bf16); with rs_part,
    G passes one rounding of g * rs to its own type (u_G; fp16: spacing 2^-24 below 2^-14, 2^-25 absolute per token).  fp32:
    the summation chain of the host rule (_n_acc) on |G rs|^T |X| + |C|, and rs's own error (_e_rs) plus its product (E)."""
    dev = gpu["device"]
    M, H, n, g0 = WGRAD_CASES[ci]
    op = WOperands(M, H, n, g0, WGRAD_LDG[ci], gdt, xdt, "real", 350 + ci, dev)
    base = torch.randn(n, H, generator=op.gen).to(dev).double()
    conv = gdt == BF16 and xdt == F16
    for trans, npart in WGRAD_REAL_CALLS:
        what = f"wgrad_tn {WGRAD_CASES[ci]} G {_name(gdt)} X {_name(xdt)} trans={trans} rs_npart={npart}"
        part = op.parts[npart] if npart else None
        part0 = part.clone() if npart else None
        C = _c_buffer(n, H, trans, base, dev)
        _ok(_wgrad_call(op, WGRAD_CASES[ci], gdt, xdt, trans, C, part, npart), what)
        C.check(what)
        op.unchanged(what)
        if npart:
            _unchanged([("rs_part", part, part0)], what)
        gs = op.g64 * _rs64(part, 512)[:, None] if npart else op.g64
        ref = base + gs.T @ op.x64
        emul = base + (_rnd(gs, gdt) if npart else gs).T @ (_rnd(op.x64, BF16) if conv else op.x64)
        unit = gs.abs().T @ op.x64.abs()
        u16 = (_U[gdt] if npart else 0.0) + (_U[BF16] if conv else 0.0)
        f32 = _n_acc(M, H) * _E * (unit + base.abs()) + ((_e_rs(npart) + _E) * unit if npart else 0.0)
        sub = 2.0 ** -25 * op.x64.abs().sum(0)[None, :].expand(n, H) if (npart and gdt == F16) else 0.0
        got = C.region.T if trans else C.region
        key = ("tcavt_wgrad_tn", f"wgrad_tn_kernel<X {_name(xdt)}, G {_name(gdt)}>" + (" rs_part" if npart else ""), _name(gdt))
        _check(got, ref, u16 * unit, 1.01 * f32 + sub + _ulp(ref, F32), what, key)
        _global(got, ref, emul, what, key)


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_lora_wgrad_a

def _gamma_pattern(H, dev):
    """recognisable per column, never 1, a different level from column 256 on"""
    h = torch.arange(H, dtype=F64)
    return (1.25 + ((h * 37) % 101) / 202 + (h >= 256) * 0.75).float().to(dev)


def _lora_a_run(dev, M, H, dt, p, npart, small_rms, seed):
    g_ = _gen(seed)
    x = _randn((M, H), g_, dev) * (0.02 if small_rms else 1.5) * (1 if small_rms else _gains(M, g_, dev))
    X = Poisoned(M, H, dt, dev, ld=H, extra_rows=3, fill=x)
    col_gain = (0.5 + torch.arange(32, dtype=F64) / 16).to(dev)[None, :]      # a different gain in each of the 32 columns
    gt = torch.zeros(M, 64, dtype=F64, device=dev)
    gt[:, :32] = _randn((M, 32), g_, dev) * col_gain * (600 if small_rms else 3)
    GT = Poisoned(M, 64, dt, dev, ld=64, extra_rows=3, fill=gt)
    gamma = _gamma_pattern(H, dev)
    part = X.region.float().pow(2).view(M, npart, H // npart).sum(-1).contiguous()   # (an input the test makes; fp32 sums)
    base = torch.randn(32, H, generator=g_).to(dev)
    dA = Guarded(32, H, F32, dev, ld=H + 16, fill=base, after=32)                    # rows 32..63 of dA are guard rows
    gam0, part0 = gamma.clone(), part.clone()
    inst = f"lora_wgrad_a_kernel p={p}" + (" small rms" if small_rms else "")
    what = f"lora_wgrad_a {M}x{H} {_name(dt)} p={p} npart={npart}" + (" small rms" if small_rms else "")
    rc = _L().tcavt_lora_wgrad_a(X.buf.data_ptr(), part.data_ptr(), npart, EPS, gamma.data_ptr(), GT.buf.data_ptr(), dA.ptr, dA.ld, M, H,
                                 p, SEED, SITE_Q, SITE_V, _dt_code(dt), _st())
    _ok(rc, what)
    dA.check(what)
    _unchanged([("x16", X.buf, X.before), ("g_t", GT.buf, GT.before), ("gamma", gamma, gam0), ("part", part, part0)], what)
    # float64: dA[a * 16 + r][h] = gamma[h] * sum_m g_t[m][a * 16 + r] * keep_a[m][h] / (1 - p) * rs[m] * x[m][h]
    rs = _rs64(part, H)[:, None]
    x64, g64, gm = X.region.double(), GT.region.double(), gamma.double()[None, :]
    n_acc, e_x = _n_acc(M, H), _e_rs(npart) + 3 * _E   # x * rs, * keep scale (fp32 quotient), the accumulator * gamma
    for a, site in ((0, SITE_Q), (1, SITE_V)):
        xs = x64 * rs * _keep(M, H, p, site, dev) * _inv_keep(p)
        ga = g64[:, 16 * a:16 * a + 16]
        ref = base[16 * a:16 * a + 16].double() + gm * (ga.T @ xs)
        emul = base[16 * a:16 * a + 16].double() + gm * (ga.T @ _rnd(xs, dt))
        unit = gm.abs() * (ga.abs().T @ xs.abs())
        f32 = n_acc * _E * (unit + base[16 * a:16 * a + 16].double().abs()) + e_x * unit
        sub = 2.0 ** -25 * gm.abs() * ga.abs().sum(0)[:, None].expand(16, H) if dt == F16 else 0.0
        key = ("tcavt_lora_wgrad_a", inst, _name(dt))
        blk = dA.region[16 * a:16 * a + 16]
        _check(blk, ref, _U[dt] * unit, 1.01 * f32 + sub + _ulp(ref, F32), f"{what} d{'qv'[a]}", key)   # the operand rounds ONCE
        _global(blk, ref, emul, f"{what} d{'qv'[a]}", key)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("ci", range(len(LORA_A_CASES)), ids=lambda i: "x".join(map(str, LORA_A_CASES[i])))
def test_lora_wgrad_a(gpu, ci, dt):
    M, H = LORA_A_CASES[ci]
    for d in (0, 1):
        p, npart = LORA_A_CALLS[(ci + d) % 5]
        _lora_a_run(gpu["device"], M, H, dt, p, npart, False, 400 + ci)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_lora_wgrad_a_small_rms(gpu, p, dt):
    """the stream of decoder layer 0 (rms ~0.02, 1 / rms ~50) under a gradient near the top of the half range: 1 / rms meets the
    stream operand, not the gradient; finite, and inside the same per-element bound"""
    _lora_a_run(gpu["device"], 200, 512, dt, p, 8, True, 450)


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_lora_down, tcavt_lora_dgrad

def _lora_down_case(dev, M, H, dt, p, regime, seed):
    g_ = _gen(seed)
    if regime == "exact":
        x, a, s = _ints((M, H), 4, g_, dev), _ints((32, H), 4, g_, dev), 0.25
    else:
        x, a, s = _randn((M, H), g_, dev) * _gains(M, g_, dev), _randn((32, H), g_, dev) * 0.05, 4.0
    X = Poisoned(M, H, dt, dev, ld=H, extra_rows=3, fill=x)
    a_cat = torch.zeros(64, H, dtype=F64, device=dev)
    a_cat[:32] = a
    A = Poisoned(64, H, dt, dev, ld=H, extra_rows=3, fill=a_cat)
    t = Guarded(M, 32, dt, dev, ld=64)                                   # columns 32..63 and the rows around are guards
    what = f"lora_down {regime} {M}x{H} {_name(dt)} p={p}"
    rc = _L().tcavt_lora_down(X.buf.data_ptr(), A.buf.data_ptr(), t.ptr, M, H, s, p, SEED, SITE_Q, SITE_V, _dt_code(dt), _st())
    _ok(rc, what)
    t.check(what)
    _unchanged([("x16", X.buf, X.before), ("a_cat", A.buf, A.before)], what)
    x64, a64 = X.region.double(), A.region.double()
    for ad, site in ((0, SITE_Q), (1, SITE_V)):
        xs = x64 * _keep(M, H, p, site, dev) * _inv_keep(p)
        aa = a64[16 * ad:16 * ad + 16]
        ref = s * (xs @ aa.T)
        got = t.region[:, 16 * ad:16 * ad + 16]
        if regime == "exact":
            assert (xs.abs() @ aa.abs().T).max().item() < 2.0 ** 24
            bad = ~(got.double() == _round(ref, dt).double())
            assert not bool(bad.any()), f"{what} adapter {ad}: {int(bad.sum())} elements differ; first {_first_bad(bad)}"
            continue
        # the masked operand is rounded once (exact for p = 0 and p = 0.5: x, 2 x); fp32: x * scale (E; the quotient is the host's),
        # H / 4 products chained per wave, three additions across the waves, the product with `scale`; one output rounding
        unit = s * (xs.abs() @ aa.abs().T)
        c = 1.0 if p not in (0.0, 0.5) else 0.0
        f32 = (H / 4 + 3 + 1 + 1) * _E * unit
        key = ("tcavt_lora_down", f"lora_down_kernel p={p}", _name(dt))
        _check(got, ref, c * _U[dt] * unit, 1.01 * f32 + _ulp(ref, dt), f"{what} adapter {ad}", key)
        _global(got, ref, _rnd(s * (_rnd(xs, dt) @ aa.T), dt), f"{what} adapter {ad}", key)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("M,H", LORA_DOWN_CASES)
def test_lora_down(gpu, M, H, dt):
    for p in (0.0, 0.5):
        _lora_down_case(gpu["device"], M, H, dt, p, "exact", 500 + M)
    for p in P_VALUES:
        _lora_down_case(gpu["device"], M, H, dt, p, "real", 520 + M)


def _lora_dgrad_case(dev, M, H, dt, p, regime, seed):
    g_ = _gen(seed)
    gt = torch.zeros(M, 64, dtype=F64, device=dev)
    aq, av = torch.zeros(H, 64, dtype=F64, device=dev), torch.zeros(H, 64, dtype=F64, device=dev)
    if regime == "exact":
        gt[:, :32], aq[:, :16], av[:, 16:32] = _ints((M, 32), 4, g_, dev), _ints((H, 16), 4, g_, dev), _ints((H, 16), 4, g_, dev)
    else:
        gt[:, :32] = _randn((M, 32), g_, dev) * _gains(M, g_, dev)
        aq[:, :16], av[:, 16:32] = _randn((H, 16), g_, dev) * 0.05, _randn((H, 16), g_, dev) * 0.05
    GT = Poisoned(M, 64, dt, dev, ld=64, extra_rows=3, fill=gt)
    AQ = Poisoned(H, 64, dt, dev, ld=64, extra_rows=3, fill=aq)
    AV = Poisoned(H, 64, dt, dev, ld=64, extra_rows=3, fill=av)
    out = Guarded(M, H, dt, dev)
    what = f"lora_dgrad {regime} {M}x{H} {_name(dt)} p={p}"
    rc = _L().tcavt_lora_dgrad(GT.buf.data_ptr(), AQ.buf.data_ptr(), AV.buf.data_ptr(), out.ptr, M, H, p, SEED, SITE_Q, SITE_V,
                               _dt_code(dt), _st())
    _ok(rc, what)
    out.check(what)   # (rows >= M, which a partial 16-token block clamps to row M - 1, are guard rows)
    _unchanged([("g_t", GT.buf, GT.before), ("aqT", AQ.buf, AQ.before), ("avT", AV.buf, AV.before)], what)
    g64 = GT.region.double()[:, :32]
    kq, kv = _keep(M, H, p, SITE_Q, dev), _keep(M, H, p, SITE_V, dev)
    pq, pv = g64 @ AQ.region.double()[:, :32].T, g64 @ AV.region.double()[:, :32].T
    ref = (kq * pq + kv * pv) * _inv_keep(p)
    if p > 0:
        both = (kq == 0) & (kv == 0)
        assert bool(both.any()) or M * H < 2048
        assert bool((out.region.float()[both] == 0).all()), f"{what}: an element dropped under both masks is not an exact zero"
    if regime == "exact":
        bad = ~(out.region.double() == _round(ref, dt).double())
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ; first {_first_bad(bad)}"
        return
    # no 16-bit rounding before the output: one MFMA of 32 products per adapter, two mask products, one addition
    unit = (kq * (g64.abs() @ AQ.region.double()[:, :32].abs().T) + kv * (g64.abs() @ AV.region.double()[:, :32].abs().T)) * _inv_keep(p)
    key = ("tcavt_lora_dgrad", f"lora_dgrad_kernel p={p}", _name(dt))
    _check(out.region, ref, 0 * ref, 1.01 * (32 + 3) * _E * unit + _ulp(ref, dt), what, key)
    _global(out.region, ref, _rnd(ref, dt), what, key)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("M,H", LORA_DGRAD_CASES)
def test_lora_dgrad(gpu, M, H, dt):
    for p in (0.0, 0.5):
        _lora_dgrad_case(gpu["device"], M, H, dt, p, "exact", 600 + M)
    for p in P_VALUES:
        _lora_dgrad_case(gpu["device"], M, H, dt, p, "real", 620 + M)


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_grad_scale_pick

def _scale_inputs(dt, dev, amax, holder, n, fill, seed):
    g_ = _gen(seed)
    a = _rnd((torch.rand(n, generator=g_).double() * 2 - 1) * amax * fill, dt).to(dt).to(dev)
    b = _rnd((torch.rand(n, generator=g_).double() * 2 - 1) * amax * fill, dt).to(dt).to(dev)
    (a if holder == "a" else b)[n - 3] = -amax   # in the last octet, negative: |.| is what counts
    return a, b


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_grad_scale_pick(gpu, dt):
    dev = gpu["device"]
    for i, (name, amax, holder, n, backoff, fill) in enumerate(_scale_cases(dt)):
        a, b = _scale_inputs(dt, dev, amax, holder, n, fill, 700 + i)
        a0, b0 = a.clone(), b.clone()
        use_b = holder == "b" or i % 2 == 0
        assert max(a.double().abs().max().item(), b.double().abs().max().item() if use_b else 0.0) == amax
        scale = _pick_scale(a, b if use_b else None, dt, dev, backoff=backoff if backoff or i % 2 else None)
        _unchanged([("g_a", a, a0), ("g_b", b, b0)], name)
        S, inv = scale.region[0, 0].item(), scale.region[0, 1].item()
        want = _expected_scale(amax, TARGET, backoff)
        assert math.frexp(S)[0] == 0.5 and S == want, (name, _name(dt), S, want)
        assert inv == 1 / S and float(np.float32(1) / np.float32(S)) == inv, (name, S, inv)
        if "overflows" in name:
            assert S == 2.0 ** 60, (name, S)      # the documented end: the exponent clamps at 60
        else:
            assert TARGET / 2 <= amax * S * 2.0 ** backoff <= TARGET, (name, amax, S)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_grad_scale_pick_zero_and_non_finite(gpu, dt):
    """all zero: S = 1.  An inf: S = 1.  A NaN is dropped by the maximum (fmaxf), so S follows the finite values beside it -- the
    NaN itself travels on through the backward and the gated optimizer skips the update, whatever S is.  The header and the
    kernel say the same."""
    dev = gpu["device"]
    z = torch.zeros(4096, dtype=dt, device=dev)
    z[5] = -0.0
    assert _pick_scale(z, None, dt, dev).region[0].tolist() == [1.0, 1.0]
    assert _pick_scale(z, z.clone(), dt, dev, backoff=4).region[0].tolist() == [1.0, 1.0]
    a, b = _scale_inputs(dt, dev, 3.0, "a", 4096, 0.9, 750)
    for holder, v in (("a", float("inf")), ("b", float("-inf"))):
        aa, bb = a.clone(), b.clone()
        (aa if holder == "a" else bb)[1000] = v
        assert _pick_scale(aa, bb, dt, dev).region[0].tolist() == [1.0, 1.0], (holder, v)
    for holder in "ab":
        aa, bb = a.clone(), b.clone()
        (aa if holder == "a" else bb)[[0, 1001, 4095]] = float("nan")
        assert _pick_scale(aa, bb, dt, dev).region[0].tolist() == [64.0, 1 / 64.0], holder       # 3 * 64 = 192 in [128, 256]
    assert _pick_scale(torch.full((8,), float("nan"), dtype=dt, device=dev), None, dt, dev).region[0].tolist() == [1.0, 1.0]


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_clip_grad_norm

def _clip(g, n, max_norm, grad_scale, scratch):
    rc = _L().tcavt_clip_grad_norm(g.ptr, n, max_norm, grad_scale, scratch.ptr, _st())
    _ok(rc, f"clip_grad_norm n={n}")


@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
@pytest.mark.parametrize("n", CLIP_N)
def test_clip_grad_norm(gpu, n, grad_scale):
    """scratch[1025] = grad_scale * ||g||: a block adds ceil(ceil(n / 1024) / 256) squares per thread (fused), six exchange
    levels and three additions; the second kernel 16 partials per lane, six levels: n_sum terms, half of it under the root,
    sqrtf (2 E), the product with grad_scale (E).  scratch[1024] = grad_scale * min(1, max_norm / (norm + 1e-6)): the addition,
    the division (2 ulps), the product.  Then every element is fp32(g * scratch[1024]), bit for bit."""
    dev = gpu["device"]
    g_ = _gen(800 + n)
    v = torch.randn(n, generator=g_).to(dev) * torch.ldexp(torch.ones(n), torch.randint(-3, 2, (n,), generator=g_)).to(dev)
    norm64 = v.double().norm().item() * grad_scale
    n_sum = -(-(-(-n // 1024)) // 256) + 9 + 16 + 6
    e_norm = (0.5 * n_sum + 3) * _E
    for max_norm in (norm64 * 4, norm64 / 3):      # one below the threshold, one above
        what = f"clip_grad_norm n={n} grad_scale={grad_scale} max_norm/norm={max_norm / norm64:.2f}"
        g = Guarded(1, n, F32, dev, ld=n + 16 + (-n) % 4, fill=v[None, :], before=4, after=4)
        scratch = Guarded(1, 1026, F32, dev, ld=1032, before=4, after=4)
        mx = float(np.float32(max_norm))
        _clip(g, n, mx, grad_scale, scratch)
        g.check(what)
        scratch.check(what + " scratch")
        norm, fac = scratch.region[0, 1025].item(), scratch.region[0, 1024].item()
        assert abs(norm - norm64) <= 1.01 * e_norm * norm64 + _ulp_of(norm64, F32), (what, norm, norm64)
        want = grad_scale * min(1.0, mx / (norm64 + 1e-6))
        e_fac = (e_norm + _E + _T + _E) if want < grad_scale else 0.0
        assert abs(fac - want) <= 1.01 * e_fac * want + (_ulp_of(want, F32) if want < grad_scale else 0.0), (what, fac, want)
        _record(("tcavt_clip_grad_norm", "sumsq_partial + clip_scale", "f32"),
                frac=max(abs(norm - norm64) / (1.01 * e_norm * norm64 + _ulp_of(norm64, F32)),
                         abs(fac - want) / (1.01 * e_fac * want + _ulp_of(want, F32))))
        assert (fac == grad_scale) == (max_norm > norm64)
        assert _same_bits(g.region[0], v * scratch.region[0, 1024]), what + ": an element is not fp32(g * scratch[1024])"
        again = Guarded(1, n, F32, dev, ld=n + 16 + (-n) % 4, fill=v[None, :], before=4, after=4)
        scratch2 = Guarded(1, 1026, F32, dev, ld=1032, before=4, after=4)
        _clip(again, n, mx, grad_scale, scratch2)
        assert _same_bits(again.region, g.region) and _same_bits(scratch2.region[0, 1024:], scratch.region[0, 1024:]), what + ": not reproducible"
    # an all-zero gradient stays zero, the factor is grad_scale
    z = Guarded(1, n, F32, dev, ld=n + 16 + (-n) % 4, fill=torch.zeros(1, n), before=4, after=4)
    scratch = Guarded(1, 1026, F32, dev, ld=1032, before=4, after=4)
    _clip(z, n, 1.0, grad_scale, scratch)
    z.check("clip_grad_norm zeros")
    assert scratch.region[0, 1024].item() == grad_scale and scratch.region[0, 1025].item() == 0.0
    assert bool((z.region == 0).all())


def test_report_worst_ratio(gpu):
    """(runs last in file order) prints the worst fractions measured in this session per (entry point, instantiation, type)"""
    for k in sorted(_WORST):
        w = _WORST[k]
        print(f"{k[0]:24s} {k[2]:5s} {k[1]:60s} " + "  ".join(f"worst {n} {w[n]:7.3f}" for n in ("frac", "r") if n in w))
