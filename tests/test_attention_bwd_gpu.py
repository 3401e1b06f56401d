"""The attention backward kernels of csrc/attn_bwd.hip and csrc/attn_bwd_check.hip against float64 on every path.

Every case calls the C entry points and checks them per element against one float64 evaluation of the operation in torch on the
GPU, computed from the same 16-bit inputs:

    S  = scale * q k^T            (per sample and query head; the heads of a group share k, v)
    P  = exp(S - lse)             keys j < min(i + 1, kv_len[b]), else 0
    dP = dO v^T,   delta = sum_d dO * att
    dS = scale * P * (dP - delta)
    dQ = dS k,   dK = sum_group dS^T q,   dV = sum_group P^T dO
    g  = RoPE^T(dQ | dK) | dV     (position = row inside the sample)

lse (fp32) and att (16-bit) are inputs of the entry points; the tests make them themselves (lse = fp32(logsumexp64), att =
round_dt(O64); the forward kernel is not part of this module, which also serves group 16).  The forms that take no lse (two-sweep
tcavt_attn_bwd_scores, the scalar kernel) are checked against P = the float64 softmax and delta = sum_j P dP.
test_formula_matches_autograd ties the formula to float64 autograd of softmax(S) v (1e-12 relative, unrounded att and lse).

_paths(entry, T, nq, nkv, lse, outputs) mirrors the host rules of attn_bwd.hip; test_paths_coverage asserts from the case
lists that every kernel and instantiation is reached in fp16 and bf16.  Cases (B, T, nq, nkv, kv_len):

| resident (tcavt_attn_bwd_resident: attn_bwd_dq_kernel + attn_bwd_dkv_res_kernel, 16-bit stores) | why |
|---|---|
| (3, 1, 4, 1, [1, 1, 0]) | T = 1, one strip; a sample without keys |
| (3, 17, 2, 2, [17, 16, 1]) | group 1; two strips (one pair); kv_len on a strip edge; Tp 64 |
| (2, 80, 4, 2, [80, 65]) | group 2; five strips (the middle strip is its own pair); Tp 128 |
| (3, 129, 8, 1, [129, 128, 33]) | group 8, two waves per head; Tp 192; nine strips |
| (2, 200, 16, 1, [200, 7]) | group 16, one wave per head |
| (1, 255, 2, 1, [255]) | T % 16 = 15 |
| (3, 256, 8, 2, [256, 170, 31]) | the product's shape; every key strip of dkv_res active |

| long (tcavt_attn_bwd_long: attn_bwd_dq_long_kernel<U> + attn_bwd_dkv_long_kernel) | why |
|---|---|
| (2, 200, 8, 2, [200, 77]) | below 256 through the chunked entry; stats bit-equal to the resident form's |
| (2, 257, 4, 2, [257, 256]) | U = 2, QC 256; the second chunk holds one query and one key |
| (2, 320, 4, 1, [320, 1]) | group 4, QC 128 |
| (3, 384, 8, 1, [384, 257, 100]) | group 8, QC 64 |
| (2, 512, 2, 2, [512, 300]) | U = 1; exactly two chunks |
| (1, 513, 16, 1, [513]) | group 16, QC 32 (17 query chunks); third key chunk of one key |
| (1, 544, 4, 2, [100]) | whole key chunks behind kv_len |
| (2, 544, 8, 2, [544, 530]) | maximum length |
| (2, 272, 4, 2, [0, 272]) | a sample without keys through the chunked kernels |

| tiled (tcavt_attn_bwd_scores + tcavt_attn_bwd_dkv + tcavt_rope_bwd_pack, fp32 g32; and the scores+gemm outputs) | why |
|---|---|
| (2, 96, 6, 2, [96, 65]) | group 3: attn_bwd_scores_kernel below 256 (one and two sweeps), dkv_res fp32 stores |
| (3, 256, 8, 2, [256, 170, 31]) | resident shortcut of tcavt_attn_bwd_scores, fp32 stores |
| (1, 300, 4, 2, [211]) | attn_bwd_scores_kernel + attn_bwd_dkv_kernel, Tp 320, one and two sweeps |
| (1, 544, 3, 1, [530]) | group 3 at maximum length |
| (2, 70, 3, 1, [70, 0]), (2, 260, 3, 1, [0, 260]) | a sample without keys through the tiled kernels, Tp <= 256 and above |

A sample with kv_len == 0 follows the forward's convention (att = 0, lse = 0); every gradient row of it must be a finite zero.

Two regimes, each case in fp16 and bf16:

- planted (bit-exact; a mask and indexing test).  K rows are 8 * h_j, h_j random +-1 codes of length 64; query i of a head is
  8 * h_t(i), t(i) <= min(i, kv_len - 1); target patterns (a different one per head and sample): diagonal, key 0, first key of the
  diagonal 32-tile, last key of the tile before it, uniform random.  K rows j >= kv_len hold 16 * h_m copies of targets in use,
  V rows are multiples of 1/16 in [-4, 4] and +-30000 behind kv_len, dO rows integers in [-2, 2] (rows i >= kv_len too: they
  attend), lse = 512.0 exactly, att = V[t(i)].  fma(4096, c2, -l2) is exactly 0 in the kernels (both products are power-of-two
  multiples of fp32(log2 e)), every other score is at most 8 * 40 = 320: P is exactly 1 on the target and underflows to 0
  elsewhere; dP on the target and delta are the same exact sum of multiples of 1/16, so dS is exactly 0.  Required: dQ = dK = 0
  everywhere, dV[j] = round_dt(sum of the dO rows whose target is j over the group's heads) bit for bit (the exact sum in fp32
  outputs), bit-zero dK / dV rows behind kv_len, stats = (512, 1, delta, 0) exactly.  (In the 16-bit outputs the dK rows have
  passed the transposed rotation: 0 * cos - 0 * sin is -0 in IEEE arithmetic where cos < 0.  Required there, bit for bit, is
  the fp32 rotation of a +0 pair with the same table entries; dV rows and every fp32 output are bit-zero.  An off-by-one causal
  mask admits a key whose score is at most 320 and underflows here as well: the realistic regime is what catches it.)
- realistic (per-element bound).  q, k ~ N(0, sigma^2), sigma in {0.5, 1, 2} by case, v, dO ~ N(0, 1) on padded rows too, K rows
  behind kv_len = 2 * a real row.  The bound is derived next to _bounds(); the global bar per dq / dk / dv block is
  rel_err(got, ref) <= 2 * rel_err(emul, ref), emul = the same float64 formula with P and dS rounded once to the 16-bit type and
  the result rounded to the output type.  stats[:, 2] within 64 * 2^-24 * sum|dO att| of float64, stats[:, 0] bit-equal to lse.
  test_adversaries: increasing / decreasing scores, a spike on the last allowed key, q = 0, under the same bounds.

Buffers: every output lies in a larger NaN-filled allocation with guard rows before and after (16-byte-aligned views); every
in-range element must come back finite, every guard element keep its bits, every input stay bit-unchanged.  Resident and long
forms: three NaN rows behind B * T in qkv, dO and att.  Tiled form: 63 pad rows of +-30000, same bits as with zeros there.

Measured worst ratios stand next to the bars and in profiles/attention_bwd_bounds.txt; test_report_worst_ratio prints this
session's (pytest -s).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
DTYPES = [F16, BF16]
SCALE = 0.125
_U = {F16: 2.0 ** -11, BF16: 2.0 ** -8}  # unit roundoff of one rounding to the 16-bit type
_E = 2.0 ** -24                          # unit roundoff of fp32
_GUARD = 3                               # NaN rows before and after every output

# ---------------------------------------------------------------------------------------------------------------------------
# Bars.  The per-element bound is (see _bounds() for the terms; all products on absolute values in float64)
#   |dV - ref|  <= _C * u * (P^T |dO|)  + 1.01 * [fp32 terms] + [fp16 subnormal term] + ulp_out(ref)
#   |dQ - ref|  <= _C * u * (|dS| |k|)  + ...      |dK - ref| <= _C * u * sum_group (|dS|^T |q|) + ...
# _C counts the 16-bit roundings on the element's path in units of u.  Every MFMA kernel of this file computes P and dS in fp32
# from fp32 accumulators (exp2 / __expf of an fp32 argument, one subtraction, two multiplications), rounds each ONCE
# (pack16x2 / to16) into the A operand of the gradient MFMA, whose other operand (dO, q, k) is an input and exact, and
# accumulates in fp32: c = 1 for dQ and dK (dS rounded once), c = 1 for dV (P rounded once).  The scalar kernel and nothing else
# keeps P and dS in fp32: c = 0.  The second-order term (the rounding acts on the fp32 value, not on the exact one) is the
# factor 1.01 on the fp32 terms.  Measured worst c (slack over u * unit, after the other terms) are in
# profiles/attention_bwd_bounds.txt and, per (entry point, kernel, type), at the end of this comment block.
_C = 1.0
# global bar: rel_err(got, ref) <= _R * rel_err(emul, ref) per dq / dk / dv block.  The emulation and the kernel differ only in
# summation order and fp32 effects (the forward module measured 1.0 .. 1.35 for the analogous ratio)
_R = 2.0
# stats[:, 2] = dO . att: 64 fp32 fused multiply-adds (16 per lane and two exchanges)
_F_DELTA = 64
# MEASURED on an MI355X, worst c / worst r per (entry point, kernels, type) over the cases, both regimes and the adversaries
# (profiles/attention_bwd_bounds.txt has every case):
#   tcavt_attn_bwd_resident  dq_kernel + dkv_res_kernel, 16-bit stores         f16 0.556 / 1.005 (adversaries 0.739 / 1.044)
#                                                                              bf16 0.713 / 1.000 (adversaries 0.714 / 1.003)
#   tcavt_attn_bwd_long      dq_long_kernel<U=1> + dkv_long_kernel             f16 0.446 / 1.000   bf16 0.568 / 1.000
#                            dq_long_kernel<U=2> + dkv_long_kernel             f16 0.585 / 1.001 (adversaries 0.687 / 1.030)
#                                                                              bf16 0.730 / 1.001 (adversaries 0.691 / 1.004)
#   tcavt_attn_bwd_scores + _dkv, fp32 g32:
#     dq_kernel + dkv_res_kernel, fp32 stores (the shortcut)                   f16 0.723 / 1.000   bf16 0.882 / 1.000
#     scores_kernel one sweep  + dkv_res_kernel, fp32 stores                   f16 0.718 / 1.000   bf16 0.842 / 1.000
#     scores_kernel two sweeps + dkv_res_kernel, fp32 stores                   f16 0.681 / 1.000   bf16 0.879 / 1.000
#     scores_kernel one sweep  + dkv_kernel                                    f16 0.665 / 1.000   bf16 0.898 / 1.001
#     scores_kernel two sweeps + dkv_kernel                                    f16 0.488 / 1.000   bf16 0.873 / 1.001
#     ... + tcavt_rope_bwd_pack (16-bit)                                       f16 <= 0.571 / 1.001   bf16 <= 0.774 / 1.001
#   tcavt_attn_bwd_scores with PT / dST / dS (one rounding each)               P^T 0.995, dS = dS^T 0.990 (bf16); 0.983, 0.956 (f16)
#   tcavt_causal_softmax_bwd_tiles / _rows (bf16)                              P 0.994, dS 0.991
#   tcavt_attn_causal_gqa_bwd (c = 0: the fp32 terms alone)                    0.013 of its bound
#   tcavt_rope_bwd_pack, tcavt_gqa_rope_bwd_pack                               0.500 of the bound (the output rounding)
# P rounded through bf16 in attn_bwd_dkv_res_kernel<fp16> (a mutant) gives c = 3.8 .. 5.7.
_WORST = {}   # (entry, kernel, type) -> dict(c=..., r=...)


def _lib():
    from tcavt_amd import capi

    return capi


def _dt_code(dt):
    capi = _lib()
    return {F32: capi.F32, BF16: capi.BF16, F16: capi.F16}[dt]


def _name(dt):
    return str(dt)[6:].replace("float", "f")


def _bits(t):
    return t.view({F32: torch.int32, F16: torch.int16, BF16: torch.int16, torch.int32: torch.int32}[t.dtype])


def _same_bits(a, b):
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _ulp(x, dt):
    """ulp of dt at |x| (float64 tensor), subnormal spacing below the normal range"""
    p, emin = {F16: (10, -14), BF16: (7, -126), F32: (23, -126)}[dt]
    _, e = torch.frexp(x)
    e = torch.where(x == 0, torch.full_like(e, emin + 1), e)
    return torch.ldexp(torch.ones_like(x), (e - 1).clamp_min(emin) - p)


def _rnd(x, dt):
    """float64 -> dt -> float64"""
    return x.float().to(dt).double()


def _last_error():
    msg = _lib().lib().tcavt_last_error()
    return msg.decode() if msg else ""


def _first_bad(bad):
    return tuple(bad.nonzero()[0].tolist())


def _case_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}x{c[3]}"


# ---------------------------------------------------------------------------------------------------------------------------
# host-rule mirror and the case lists

def _paths(entry, T, nq, nkv, lse=True, outputs=()):
    """The kernels a call of `entry` launches, by the rules of attn_bwd.hip; None when the entry point refuses the shape.
    outputs (tcavt_attn_bwd_scores only): which of dQ, stats, dS, PT are requested."""
    if nkv <= 0 or nq <= 0 or nq % nkv or T <= 0:
        return None
    group = nq // nkv
    Tp = (T + 63) & ~63
    if entry == "resident":
        if T > 256 or 16 % group:
            return None
        return ["attn_bwd_dq_kernel/store16", "attn_bwd_dkv_res_kernel/store16"]
    if entry == "long":
        if T > 544 or 16 % group:
            return None
        return [f"attn_bwd_dq_long_kernel<U={min(group, 2)}>", "attn_bwd_dkv_long_kernel"]
    if entry == "scores":
        out = set(outputs)
        if lse and out == {"dQ", "stats"} and Tp <= 256 and 16 % group == 0:
            return ["attn_bwd_dq_kernel/store32"]
        return ["attn_bwd_scores_kernel/" + ("one sweep" if lse else "two sweeps")]
    if entry == "dkv":
        return ["attn_bwd_dkv_res_kernel/store32" if Tp <= 256 else "attn_bwd_dkv_kernel"]
    if entry == "scalar":
        return ["attn_causal_gqa_bwd_kernel"] if T <= 280 else None
    return {"softmax_tiles": ["causal_softmax_bwd_tiles_kernel"], "softmax_rows": ["causal_softmax_bwd_rows_kernel"],
            "rope_pack": ["rope_bwd_pack_kernel"], "gqa_pack": ["gqa_rope_bwd_pack_kernel"]}[entry]


def _long_chunks(T, nq, nkv):
    """(QC, query chunks, key chunks) of tcavt_attn_bwd_long"""
    group = nq // nkv
    QC = 256 * min(group, 2) // group
    return QC, -(-T // QC), -(-T // 256)


RESIDENT_CASES = [
    (3, 1, 4, 1, [1, 1, 0]),
    (3, 17, 2, 2, [17, 16, 1]),
    (2, 80, 4, 2, [80, 65]),
    (3, 129, 8, 1, [129, 128, 33]),
    (2, 200, 16, 1, [200, 7]),
    (1, 255, 2, 1, [255]),
    (3, 256, 8, 2, [256, 170, 31]),
]
LONG_CASES = [
    (2, 200, 8, 2, [200, 77]),
    (2, 257, 4, 2, [257, 256]),
    (2, 320, 4, 1, [320, 1]),
    (3, 384, 8, 1, [384, 257, 100]),
    (2, 512, 2, 2, [512, 300]),
    (1, 513, 16, 1, [513]),
    (1, 544, 4, 2, [100]),
    (2, 544, 8, 2, [544, 530]),
    (2, 272, 4, 2, [0, 272]),
]
TILED_CASES = [
    (2, 96, 6, 2, [96, 65]),
    (3, 256, 8, 2, [256, 170, 31]),
    (1, 300, 4, 2, [211]),
    (1, 544, 3, 1, [530]),
    (2, 70, 3, 1, [70, 0]),
    (2, 260, 3, 1, [0, 260]),
]
SCALAR_CASES = [RESIDENT_CASES[0], RESIDENT_CASES[2], RESIDENT_CASES[3]]  # bf16 only: the kernel has no fp16 form
SOFTMAX_CASES = [TILED_CASES[0], TILED_CASES[2]]                          # bf16 only
ADVERSARY_CASES = [("resident", RESIDENT_CASES[3]), ("resident", RESIDENT_CASES[5]), ("long", LONG_CASES[1]), ("long", LONG_CASES[7])]
ALL_CASES = RESIDENT_CASES + LONG_CASES + TILED_CASES
# the tiled form's calls per case: (lse given, outputs of tcavt_attn_bwd_scores)
TILED_CALLS = [(True, ("dQ", "stats")), (False, ("dQ", "stats")), (True, ("dQ", "dS", "PT")), (False, ("dQ", "dS", "PT"))]


def _launched():
    """(kernel, type) of every launch the case lists make"""
    seen = set()
    for dt in DTYPES:
        n = _name(dt)
        for c in RESIDENT_CASES:
            seen |= {(k, n) for k in _paths("resident", c[1], c[2], c[3])}
        for c in LONG_CASES:
            seen |= {(k, n) for k in _paths("long", c[1], c[2], c[3])}
        for c in TILED_CASES:
            for lse, outs in TILED_CALLS:
                seen |= {(k, n) for k in _paths("scores", c[1], c[2], c[3], lse, outs)}
            seen |= {(k, n) for k in _paths("dkv", c[1], c[2], c[3])}
            seen.add(("rope_bwd_pack_kernel", n))
    for c in SCALAR_CASES:
        seen |= {(k, "bf16") for k in _paths("scalar", c[1], c[2], c[3])}
    seen |= {("causal_softmax_bwd_tiles_kernel", "bf16"), ("causal_softmax_bwd_rows_kernel", "bf16"), ("gqa_rope_bwd_pack_kernel", "bf16")}
    return seen


def test_paths_coverage():
    """from the case lists alone: every kernel and instantiation is reached, in fp16 and bf16 where it has both forms, with
    every group the host rule admits and at the lengths where a rule switches"""
    both = ["attn_bwd_dq_kernel/store16", "attn_bwd_dq_kernel/store32", "attn_bwd_dkv_res_kernel/store16",
            "attn_bwd_dkv_res_kernel/store32", "attn_bwd_dq_long_kernel<U=1>", "attn_bwd_dq_long_kernel<U=2>",
            "attn_bwd_dkv_long_kernel", "attn_bwd_scores_kernel/one sweep", "attn_bwd_scores_kernel/two sweeps",
            "attn_bwd_dkv_kernel", "rope_bwd_pack_kernel"]
    bf16_only = ["attn_causal_gqa_bwd_kernel", "causal_softmax_bwd_tiles_kernel", "causal_softmax_bwd_rows_kernel",
                 "gqa_rope_bwd_pack_kernel"]
    want = {(k, n) for k in both for n in ("f16", "bf16")} | {(k, "bf16") for k in bf16_only}
    assert _launched() == want, (sorted(want - _launched()), sorted(_launched() - want))
    for B, T, nq, nkv, kv in ALL_CASES + SCALAR_CASES:
        assert 1 <= B <= 3 and 1 <= T <= 544 and len(kv) == B and all(0 <= n <= T for n in kv)
    assert {c[2] // c[3] for c in RESIDENT_CASES} == {1, 2, 4, 8, 16}
    assert {c[2] // c[3] for c in LONG_CASES} == {1, 2, 4, 8, 16}
    assert {_long_chunks(c[1], c[2], c[3])[0] for c in LONG_CASES} == {256, 128, 64, 32}
    assert _long_chunks(513, 16, 1) == (32, 17, 3) and _long_chunks(257, 4, 2) == (256, 2, 2) and _long_chunks(512, 2, 2) == (256, 2, 2)
    assert _long_chunks(200, 8, 2)[1:] == (2, 1)
    Ts = [c[1] for c in RESIDENT_CASES]
    assert 1 in Ts and 256 in Ts and any(T % 16 == 15 for T in Ts) and any(((T + 15) // 16) % 2 == 1 and T > 16 for T in Ts)
    assert {(c[1] + 63) & ~63 for c in RESIDENT_CASES} >= {64, 128, 192, 256}
    assert any(0 in c[4] for c in RESIDENT_CASES) and any(c[1] == 544 and max(c[4]) <= 256 for c in LONG_CASES)
    assert any(0 in c[4] for c in LONG_CASES) and {(c[1] + 63) & ~63 <= 256 for c in TILED_CASES if 0 in c[4]} == {True, False}
    # the tiled form: group 3 (never resident) below and above 256, the shortcut, and Tp > 256 with a resident-capable group
    assert _paths("scores", 96, 6, 2, True, ("dQ", "stats")) == ["attn_bwd_scores_kernel/one sweep"]
    assert _paths("scores", 256, 8, 2, True, ("dQ", "stats")) == ["attn_bwd_dq_kernel/store32"]
    assert _paths("scores", 256, 8, 2, True, ("dQ", "dS", "PT")) == ["attn_bwd_scores_kernel/one sweep"]
    assert _paths("scores", 300, 4, 2, True, ("dQ", "stats")) == ["attn_bwd_scores_kernel/one sweep"]
    assert _paths("dkv", 256, 8, 2) == ["attn_bwd_dkv_res_kernel/store32"] and _paths("dkv", 257, 8, 2) == ["attn_bwd_dkv_kernel"]
    for entry, c in ADVERSARY_CASES:
        assert _paths(entry, c[1], c[2], c[3]) is not None
    assert all(c[1] <= 280 for c in SCALAR_CASES)


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 reference, its emulation floor and the per-element bound

def _heads(qkv, dO, B, T, nq, nkv):
    g = nq // nkv
    x = qkv.double().view(B, T, nq + 2 * nkv, 64)
    q = x[:, :, :nq].permute(0, 2, 1, 3)
    k = x[:, :, nq:nq + nkv].permute(0, 2, 1, 3).repeat_interleave(g, dim=1)
    v = x[:, :, nq + nkv:].permute(0, 2, 1, 3).repeat_interleave(g, dim=1)
    do = dO.double().view(B, T, nq, 64).permute(0, 2, 1, 3)
    return q, k, v, do


def _mask(kv_len, T):
    i = torch.arange(T, device=kv_len.device)
    return ((i[None, :] <= i[:, None])[None] & (i[None, None, :] < kv_len[:, None, None]))[:, None]  # [B, 1, T, T]


def _softmax_stats(q, k, v, m):
    """float64 forward: lse (0 for a query without a key) and O, [B, nq, T] and [B, nq, T, 64]"""
    s = ((q @ k.transpose(-1, -2)) * SCALE).masked_fill(~m, float("-inf"))
    zero = torch.zeros((), dtype=F64, device=q.device)
    lse = torch.where(m.any(-1), torch.logsumexp(s, -1), zero)
    p = torch.where(m, torch.exp(s.masked_fill(~m, 0.0) - lse[..., None]), zero)
    return lse, p @ v


def _flat(t, B, T):
    return t.permute(0, 2, 1, 3).reshape(B * T, -1)


def _gsum(t, B, nq, nkv):
    return t.view(B, nkv, nq // nkv, *t.shape[2:]).sum(2)


def _unrotate(x, cos, sin, n_rot_heads, T):
    """the transposed rotation on the first n_rot_heads heads of x [M, heads * 64] (float64); position = row % T"""
    M = x.shape[0]
    h = x.view(M, -1, 64).clone()
    pos = torch.arange(M, device=x.device) % T
    cs, sn = cos.double()[pos][:, None, :], sin.double()[pos][:, None, :]
    a, b = h[:, :n_rot_heads, :32].clone(), h[:, :n_rot_heads, 32:].clone()
    h[:, :n_rot_heads, :32] = a * cs + b * sn
    h[:, :n_rot_heads, 32:] = b * cs - a * sn
    return h.view(M, -1)


def _rot_bound(bnd, ref, cos, sin, n_rot_heads, T):
    """bound of the rotated element: |cos| b_a + |sin| b_b + 2^-23 (|a cos| + |b sin|): two fp32 products and one sum
    (-ffp-contract=off: three roundings, 2^-24 each on at most |a cos| + |b sin|)"""
    M = ref.shape[0]
    bh, rh = bnd.view(M, -1, 64).clone(), ref.view(M, -1, 64)
    pos = torch.arange(M, device=ref.device) % T
    cs, sn = cos.double()[pos][:, None, :].abs(), sin.double()[pos][:, None, :].abs()
    ba, bb = bh[:, :n_rot_heads, :32].clone(), bh[:, :n_rot_heads, 32:].clone()
    a, b = rh[:, :n_rot_heads, :32].abs(), rh[:, :n_rot_heads, 32:].abs()
    bh[:, :n_rot_heads, :32] = cs * ba + sn * bb + 2.0 ** -23 * (a * cs + b * sn)
    bh[:, :n_rot_heads, 32:] = cs * bb + sn * ba + 2.0 ** -23 * (b * cs + a * sn)
    return bh.view(M, -1)


class Ref:
    """One float64 evaluation for one set of inputs and one form (with lse / att, or without)."""

    def __init__(self, inp, with_lse, dt16, keep_tiles=False):
        B, T, nq, nkv = inp.B, inp.T, inp.nq, inp.nkv
        q, k, v, do = _heads(inp.qkv[:B * T], inp.dO[:B * T], B, T, nq, nkv)
        m = _mask(inp.kv_len, T)
        zero = torch.zeros((), dtype=F64, device=q.device)
        S = (q @ k.transpose(-1, -2)) * SCALE
        if with_lse:
            lse = inp.lse.double().view(B, nq, T)
            att = inp.att[:B * T].double().view(B, T, nq, 64).permute(0, 2, 1, 3)
        else:
            lse = torch.where(m.any(-1), torch.logsumexp(S.masked_fill(~m, float("-inf")), -1), zero)
        P = torch.where(m, torch.exp(S.masked_fill(~m, 0.0) - lse[..., None]), zero)
        dP = do @ v.transpose(-1, -2)
        delta = (do * att).sum(-1) if with_lse else (P * dP).sum(-1)
        dS = SCALE * P * (dP - delta[..., None])
        self.delta, self.lse = delta, lse
        self.delta_abs = (do * att).abs().sum(-1) if with_lse else None

        def grads(Pm, dSm):
            return torch.cat([_flat(dSm @ k, B, T), _flat(_gsum(dSm.transpose(-1, -2) @ q, B, nq, nkv), B, T),
                              _flat(_gsum(Pm.transpose(-1, -2) @ do, B, nq, nkv), B, T)], 1)

        self.g = grads(P, dS)                                      # un-rotated, [M, (nq + 2 nkv) * 64]
        self.g_emul = grads(_rnd(P, dt16), _rnd(dS, dt16))         # P and dS rounded once
        # ---- the per-element bound (un-rotated, without the output ulp), split into its u-unit and the rest
        # fp32 relative error of P = exp2(fma(s, c2, -l2)) (* 1 / sum): the score is an MFMA sum of 64 products (64 * 2^-24 on
        # sum|q k|), c2 and l2 are rounded products (one each on |S| and |lse|), the fma rounds once on |S - lse| <= |S| + |lse|,
        # exp2 / __expf are accurate to 2 ulps of the result and amplify the argument's error by ln 2 < 1, the product with
        # 1 / sum is one more: (64 + 4) * 2^-24 * scale * sum|q k| + 4 * 2^-24 * |lse| + 8 * 2^-24.  Without lse the row maximum
        # and the row sum are the kernel's own: T additions of positive terms, T * 2^-24 relative
        qa, ka, va, da = q.abs(), k.abs(), v.abs(), do.abs()
        sabs = SCALE * (qa @ ka.transpose(-1, -2))
        epsP = _E * (68 * sabs + 4 * lse.abs()[..., None] + 8 + (0 if with_lse else T))
        # fp32 absolute error of dS = scale * P * (dP - delta): dP is an MFMA sum of 64 products (64 * 2^-24 * |dO| |v|^T = D);
        # delta = dO . att is 64 fused multiply-adds (64 * 2^-24 * sum|dO att|), or, without lse, a running sum over the T keys of
        # P dP, each term with dP's own error ((T + 64 + 8) * 2^-24 * sum_j P D); the subtraction and the two products round
        # once each on |dP| + |delta| <= D + |delta| (4 * 2^-24 with the constant scale)
        D = da @ va.transpose(-1, -2)
        if with_lse:
            e_delta = 64 * self.delta_abs
        else:
            e_delta = (T + 72) * (P * D).sum(-1)
        E_S = epsP * dS.abs() + _E * SCALE * P * (68 * D + (e_delta + 4 * delta.abs())[..., None])
        E_P = epsP * P
        mf = m.double().expand(B, nq, T, T)
        dSa = dS.abs()
        # u-units: what one rounding of dS (P) to the 16-bit type can move the element by, per unit roundoff
        self.unit = torch.cat([_flat(dSa @ ka, B, T), _flat(_gsum(dSa.transpose(-1, -2) @ qa, B, nq, nkv), B, T),
                               _flat(_gsum(P.transpose(-1, -2) @ da, B, nq, nkv), B, T)], 1)
        # fp32 summation of the gradient products: the MFMA accumulators of an element see at most T (dQ) or T * group (dK, dV)
        # terms, plus the propagated fp32 error of dS / P
        grp = nq // nkv
        nterm = torch.cat([torch.full((nq * 64,), float(T), dtype=F64), torch.full((2 * nkv * 64,), float(T * grp), dtype=F64)]).to(q.device)
        self.f32 = _E * nterm * self.unit + torch.cat(
            [_flat(E_S @ ka, B, T), _flat(_gsum(E_S.transpose(-1, -2) @ qa, B, nq, nkv), B, T),
             _flat(_gsum(E_P.transpose(-1, -2) @ da, B, nq, nkv), B, T)], 1)
        # fp16 only: a P or dS below 2^-14 is subnormal in fp16, spacing 2^-24: 2^-25 absolute per attended term
        self.sub = 2.0 ** -25 * torch.cat([_flat(mf @ ka, B, T), _flat(_gsum(mf.transpose(-1, -2) @ qa, B, nq, nkv), B, T),
                                           _flat(_gsum(mf.transpose(-1, -2) @ da, B, nq, nkv), B, T)], 1)
        if keep_tiles:
            self.P, self.dS, self.E_P, self.E_S, self.m = P, dS, E_P, E_S, m

    def bound_parts(self, dt16, c):
        """(unit, rest): |got - ref| <= c * u * unit + rest, un-rotated, no output ulp"""
        rest = 1.01 * self.f32 + (self.sub if dt16 == F16 and c > 0 else 0.0)
        return _U[dt16] * self.unit, rest


def _record(key, **kw):
    w = _WORST.setdefault(key, {})
    for k, v in kw.items():
        w[k] = max(w.get(k, -1.0), v)


def _check_elements(got, ref, unit, rest, c, what, key):
    """|got - ref| <= c * unit + rest per element; records the worst c = (|got - ref| - rest) / unit"""
    g = got.double()
    assert torch.isfinite(g).all(), f"{what}: {int((~torch.isfinite(g)).sum())} non-finite (unwritten) elements"
    d = (g - ref).abs()
    slack = d - rest
    pos = unit > 0
    worst = max((slack[pos] / unit[pos]).max().item(), 0.0) if bool(pos.any()) else 0.0
    frac = (d / (c * unit + rest).clamp_min(1e-300)).max().item()
    _record(key, c=worst, frac=frac)
    print(f"c {what}: {worst:.3f}  (fraction of the whole bound {frac:.3f})")
    bad = d > c * unit + rest
    if bool(bad.any()):
        i = _first_bad(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of bound (worst c {worst:.3f}); first {i}: got {g[i].item()!r} "
                             f"ref {ref[i].item()!r} allowed {(c * unit + rest)[i].item():.3e}")


def _blocks(nq, nkv):
    return (("dq", 0, nq * 64), ("dk", nq * 64, (nq + nkv) * 64), ("dv", (nq + nkv) * 64, (nq + 2 * nkv) * 64))


def _check_global(got, ref, emul, nq, nkv, what, key):
    """rel_err(got, ref) <= _R * rel_err(emul, ref) per dq / dk / dv block"""
    for name, lo, hi in _blocks(nq, nkv):
        r, g, e = ref[:, lo:hi], got[:, lo:hi].double(), emul[:, lo:hi]
        n = r.norm().item()
        if n == 0:  # (T = 1: dS = 0, no relative error to speak of; the per-element bound has judged the block)
            continue
        eg, ee = ((g - r).norm() / n).item(), ((e - r).norm() / n).item()
        if ee > 0:
            _record(key, r=eg / ee)
            print(f"r {what} {name}: {eg / ee:.3f}  (rel {eg:.3e}, emulation floor {ee:.3e})")
        assert eg <= _R * ee, f"{what} {name}: rel {eg:.3e} > {_R} * emulation floor {ee:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------
# inputs

class Inputs:
    """qkv [B * T (+ pad), ncols], dO, att [B * T (+ pad), nq * 64] of dt; lse fp32 [B * nq * T]; kv_len int32; cos / sin"""

    def __init__(self, case, dt, dev, x, do, att=None, lse=None, tgt=None):
        from tcavt_amd.config import LlamaShape
        from tcavt_amd.rope import rope_tables

        self.B, self.T, self.nq, self.nkv, self.kv = case
        self.case, self.dt, self.dev = case, dt, dev
        B, T, nq, nkv = case[:4]
        self.M, self.ncols = B * T, (nq + 2 * nkv) * 64
        self.kv_len = torch.tensor(case[4], dtype=torch.int32, device=dev)
        self.qkv = x.reshape(self.M, self.ncols).to(dt).to(dev)
        self.dO = do.reshape(self.M, nq * 64).to(dt).to(dev)
        self.cos, self.sin = (t.to(dev) for t in rope_tables(LlamaShape(), T))
        self.tgt = tgt
        if att is None:  # the forward in float64 from the rounded inputs: lse = fp32(logsumexp64), att = round_dt(O64)
            q, k, v, _ = _heads(self.qkv, self.dO, B, T, nq, nkv)
            l64, o64 = _softmax_stats(q, k, v, _mask(self.kv_len, T))
            self.lse64, self.o64 = l64, o64
            self.lse = l64.float().reshape(-1).contiguous()
            self.att = _flat(o64, B, T).float().to(dt).contiguous()
        else:
            self.att = att.reshape(self.M, nq * 64).to(dt).to(dev)
            self.lse = lse.reshape(-1).float().to(dev)

    def padded(self, rows, fill):
        """copies of qkv, dO, att with `rows` rows behind B * T: NaN, zeros, or (fill = 'big') +-30000"""
        out = []
        for t in (self.qkv, self.dO, self.att):
            p = torch.empty(t.shape[0] + rows, t.shape[1], dtype=t.dtype, device=t.device)
            p[:t.shape[0]] = t
            if fill == "big":
                sign = (torch.arange(rows * t.shape[1], device=t.device).view(rows, -1) % 2) * 2 - 1
                p[t.shape[0]:] = (30000.0 * sign).to(t.dtype)
            else:
                p[t.shape[0]:] = fill
            out.append(p)
        return out


def _codes(n, g):
    return (torch.randint(0, 2, (n, 64), generator=g) * 2 - 1).float()


def _planted(case, ci, dt, dev):
    """Inputs of the planted regime and the expected dV [B * T, nkv * 64] and delta [B, nq, T] (float64, exact)"""
    B, T, nq, nkv, kv = case
    grp = nq // nkv
    g = torch.Generator().manual_seed(1000 + ci)
    x = torch.zeros(B, T, nq + 2 * nkv, 64)
    do = torch.randint(-2, 3, (B, T, nq, 64), generator=g).float()
    do[:, :, :, 0] = 1.0  # (no dO row is all zero)
    att = torch.zeros(B, T, nq, 64)
    tgt = torch.full((B, T, nq), -1, dtype=torch.long)
    dv = torch.zeros(B, T, nkv, 64, dtype=F64)
    i = torch.arange(T)
    for b in range(B):
        n = kv[b]
        ip = i.clamp_max(n - 1)
        first = 32 * (ip // 32)
        pats = [ip, torch.zeros_like(ip), first, (first - 1).clamp_min(0)]
        for h in range(nkv):
            code = _codes(T, g)
            if n > 1:
                dots = code[:n] @ code[:n].T
                dots.fill_diagonal_(-64)
                assert dots.max().item() <= 40, f"planted codes too close: dot {dots.max().item()}"  # 8 * 40 = 320 << 512
            # padded K rows: double-weight copies of the targets that the rows behind them ask for
            src = torch.stack([p[-1] for p in pats])[i % 4] if n > 0 else i
            x[b, :, nq + h] = torch.where((i < n)[:, None], 8 * code, 16 * code[src])
            v = torch.randint(-64, 65, (T, 64), generator=g).float() / 16
            sign = (torch.randint(0, 2, (T, 64), generator=g) * 2 - 1).float()
            x[b, :, nq + nkv + h] = torch.where((i < n)[:, None], v, 30000.0 * sign)
            for hq in range(h * grp, (h + 1) * grp):
                if n == 0:
                    x[b, :, hq] = 8 * _codes(T, g)
                    continue
                rnd = (torch.rand(T, generator=g) * (ip + 1).float()).long().clamp_max(ip)
                t = (pats + [rnd])[(hq + b + ci) % 5]
                assert bool((t <= ip).all()) and bool((t >= 0).all())
                tgt[b, :, hq] = t
                x[b, :, hq] = 8 * code[t]
                att[b, :, hq] = v[t]
                dv[b, :, h].index_add_(0, t, do[b, :, hq].double())
    has = (tgt >= 0).permute(0, 2, 1)
    lse = torch.where(has, 512.0, 0.0)
    inp = Inputs(case, dt, dev, x, do, att=att, lse=lse, tgt=tgt.to(dev))
    assert torch.equal(inp.qkv.float().cpu()[:, : (nq + nkv) * 64], x.view(B * T, -1)[:, : (nq + nkv) * 64])  # q, k exact in dt
    assert torch.equal(inp.att.float().cpu(), att.view(B * T, -1)) and torch.equal(inp.dO.float().cpu(), do.view(B * T, -1))
    delta = (do.double() * att.double()).sum(-1).permute(0, 2, 1)
    return inp, dv.view(B * T, nkv * 64).to(dev), delta.to(dev)


def _pad_rows(x, case, g):
    """rows j >= kv_len of the K block of x [B, T, nq + 2 nkv, 64]: 2 * a real row (V and dO stay N(0, 1) there)"""
    B, T, nq, nkv, kv = case
    i = torch.arange(T)
    for b in range(B):
        n = kv[b]
        pad = (i >= n)[:, None, None]
        src = i % n if n > 0 else i
        x[b, :, nq:nq + nkv] = torch.where(pad, 2 * x[b, src, nq:nq + nkv], x[b, :, nq:nq + nkv])
    return x


def _sigma(case):
    return (0.5, 1.0, 2.0)[(case[1] + case[2]) % 3]


def _realistic(case, dt, dev):
    B, T, nq, nkv, kv = case
    g = torch.Generator().manual_seed(2000 + T * 17 + nq)
    x = torch.randn(B, T, nq + 2 * nkv, 64, generator=g)
    x[:, :, : nq + nkv] *= _sigma(case)
    do = torch.randn(B, T, nq, 64, generator=g)
    return Inputs(case, dt, dev, _pad_rows(x, case, g), do)


def _adversary(kind, case, dt, dev):
    B, T, nq, nkv, kv = case
    g = torch.Generator().manual_seed(T + len(kind))
    x = torch.randn(B, T, nq + 2 * nkv, 64, generator=g)
    do = torch.randn(B, T, nq, 64, generator=g)
    u = torch.randn(64, generator=g)
    u = u / u.norm() * 8  # q . k = 64 ramp, scaled score 8 ramp
    j = torch.arange(T).float()
    if kind in ("increasing", "decreasing"):  # the scores move by 40 nats over the keys
        ramp = (j if kind == "increasing" else T - 1 - j) * (40.0 / (8 * T))
        x[:, :, :nq] = u + 0.05 * x[:, :, :nq]
        x[:, :, nq:nq + nkv] = ramp[None, :, None, None] * u + 0.05 * x[:, :, nq:nq + nkv]
    elif kind == "spike":  # q_i = k_i: the row's own (last allowed) key scores 0.125 |k_i|^2 ~ 18, the others N(0, 2.25^2)
        x[:, :, nq:nq + nkv] *= 1.5
        x[:, :, :nq] = x[:, :, nq:nq + nkv].repeat_interleave(nq // nkv, dim=2)
    elif kind == "zero_q":
        x[:, :, :nq] = 0.0
    return Inputs(case, dt, dev, _pad_rows(x, case, g), do)


# ---------------------------------------------------------------------------------------------------------------------------
# launching with poisoned buffers

class Guarded:
    """rows x cols of dtype inside a NaN-filled allocation with _GUARD rows before and after (zero-initialised inside when the
    output's contract asks for it)"""

    def __init__(self, rows, cols, dtype, dev, zero=False):
        self.buf = torch.full((rows + 2 * _GUARD, cols), float("nan"), dtype=dtype, device=dev)
        self.view = self.buf[_GUARD:_GUARD + rows]
        if zero:
            self.view.zero_()
        assert self.view.data_ptr() % 16 == 0
        self.keep = self.buf.clone()
        self.rows = rows

    def guards_ok(self):
        lo, hi = slice(0, _GUARD), slice(_GUARD + self.rows, None)
        return _same_bits(self.buf[lo], self.keep[lo]) and _same_bits(self.buf[hi], self.keep[hi])

    def untouched(self):
        return _same_bits(self.buf, self.keep)


def _snapshot(inp, bufs):
    return [t.clone() for t in bufs] + [inp.lse.clone(), inp.cos.clone(), inp.sin.clone(), inp.kv_len.clone()]


def _unchanged(inp, bufs, snap, what):
    now = list(bufs) + [inp.lse, inp.cos, inp.sin, inp.kv_len]
    for t, s, nm in zip(now, snap, ("qkv", "dO", "att", "lse", "cos", "sin", "kv_len")):
        assert _same_bits(t, s), f"{what}: input {nm} modified"


def _two_launch(entry, inp, what, fill=float("nan")):
    """tcavt_attn_bwd_resident / _long on inputs with three `fill` rows behind B * T -> (g16 [M, ncols], stats [B nq T, 4])"""
    capi = _lib()
    B, T, nq, nkv = inp.case[:4]
    bufs = inp.padded(3, fill)
    snap = _snapshot(inp, bufs)
    g = Guarded(inp.M, inp.ncols, inp.dt, inp.dev)
    st = Guarded(B * nq * T, 4, F32, inp.dev)
    fn = getattr(capi.lib(), "tcavt_attn_bwd_" + entry)
    rc = fn(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), inp.lse.data_ptr(), g.view.data_ptr(), st.view.data_ptr(),
            inp.cos.data_ptr(), inp.sin.data_ptr(), inp.kv_len.data_ptr(), B, T, nq, nkv, 64, SCALE, _dt_code(inp.dt), capi.stream_ptr())
    torch.cuda.synchronize()
    capi.check(rc, what)
    assert g.guards_ok() and st.guards_ok(), f"{what}: write outside g_qkv16 / stats"
    assert torch.isfinite(g.view).all(), f"{what}: {int((~torch.isfinite(g.view)).sum())} non-finite (unwritten) gradient elements"
    assert torch.isfinite(st.view).all(), f"{what}: non-finite (unwritten) stats"
    _unchanged(inp, bufs, snap, what)
    return g.view, st.view


def _tiled(inp, with_lse, what, fill):
    """tcavt_attn_bwd_scores (dQ + stats) + tcavt_attn_bwd_dkv + tcavt_rope_bwd_pack on inputs with 63 `fill` pad rows
    -> (g32 [M, ncols] fp32, stats, g16 [M, ncols])"""
    capi = _lib()
    L = capi.lib()
    B, T, nq, nkv = inp.case[:4]
    Tp = (T + 63) & ~63
    bufs = inp.padded(63, fill)
    snap = _snapshot(inp, bufs)
    g32 = Guarded(inp.M, inp.ncols, F32, inp.dev)
    st = Guarded(B * nq * T, 4, F32, inp.dev)
    g16 = Guarded(inp.M, inp.ncols, inp.dt, inp.dev)
    rc = L.tcavt_attn_bwd_scores(bufs[0].data_ptr(), bufs[1].data_ptr(), None, None, None, g32.view.data_ptr(), inp.ncols,
                                 st.view.data_ptr(), inp.kv_len.data_ptr(), B, T, Tp, nq, nkv, 64, SCALE, _dt_code(inp.dt),
                                 inp.lse.data_ptr() if with_lse else None, bufs[2].data_ptr() if with_lse else None, capi.stream_ptr())
    torch.cuda.synchronize()
    capi.check(rc, what + " scores")
    assert torch.isfinite(g32.view[:, :nq * 64]).all(), f"{what}: non-finite (unwritten) dQ"
    assert bool(torch.isnan(g32.view[:, nq * 64:]).all()), f"{what}: tcavt_attn_bwd_scores wrote into the k / v columns"
    rc = L.tcavt_attn_bwd_dkv(bufs[0].data_ptr(), bufs[1].data_ptr(), st.view.data_ptr(), g32.view.data_ptr(), inp.kv_len.data_ptr(),
                              B, T, Tp, nq, nkv, 64, SCALE, _dt_code(inp.dt), capi.stream_ptr())
    torch.cuda.synchronize()
    capi.check(rc, what + " dkv")
    rc = L.tcavt_rope_bwd_pack(g32.view.data_ptr(), g16.view.data_ptr(), inp.cos.data_ptr(), inp.sin.data_ptr(), inp.M, inp.ncols,
                               (nq + nkv) * 64, T, _dt_code(inp.dt), capi.stream_ptr())
    torch.cuda.synchronize()
    capi.check(rc, what + " pack")
    for o, nm in ((g32, "g32"), (st, "stats"), (g16, "g_qkv16")):
        assert o.guards_ok(), f"{what}: write outside {nm}"
        assert torch.isfinite(o.view).all(), f"{what}: non-finite (unwritten) elements in {nm}"
    _unchanged(inp, bufs, snap, what)
    return g32.view, st.view, g16.view


def _scores_gemm(inp, with_lse, what):
    """tcavt_attn_bwd_scores with dQ, dS, PT, dST (no stats) -> (dQ fp32 [M, nq * 64 + 64] view, dS, PT, dST)"""
    capi = _lib()
    B, T, nq, nkv = inp.case[:4]
    Tp = (T + 63) & ~63
    bufs = inp.padded(63, 0.0)
    snap = _snapshot(inp, bufs)
    ld = nq * 64 + 64  # a leading dimension wider than the heads: the 64 columns behind them must stay NaN
    dq = Guarded(inp.M, ld, F32, inp.dev)
    dS = Guarded(B * nq * T, Tp, inp.dt, inp.dev, zero=True)
    PT = Guarded(B * nq * Tp, Tp, inp.dt, inp.dev, zero=True)
    dST = Guarded(B * nq * Tp, Tp, inp.dt, inp.dev, zero=True)
    rc = capi.lib().tcavt_attn_bwd_scores(bufs[0].data_ptr(), bufs[1].data_ptr(), dS.view.data_ptr(), PT.view.data_ptr(),
                                          dST.view.data_ptr(), dq.view.data_ptr(), ld, None, inp.kv_len.data_ptr(), B, T, Tp, nq, nkv,
                                          64, SCALE, _dt_code(inp.dt), inp.lse.data_ptr() if with_lse else None,
                                          bufs[2].data_ptr() if with_lse else None, capi.stream_ptr())
    torch.cuda.synchronize()
    capi.check(rc, what)
    for o, nm in ((dq, "dQ"), (dS, "dS"), (PT, "PT"), (dST, "dST")):
        assert o.guards_ok(), f"{what}: write outside {nm}"
    assert torch.isfinite(dq.view[:, :nq * 64]).all() and bool(torch.isnan(dq.view[:, nq * 64:]).all()), f"{what}: dQ columns"
    for o, nm in ((dS, "dS"), (PT, "PT"), (dST, "dST")):
        assert torch.isfinite(o.view).all(), f"{what}: non-finite {nm}"
    _unchanged(inp, bufs, snap, what)
    return dq.view[:, :nq * 64], dS.view, PT.view, dST.view


# ---------------------------------------------------------------------------------------------------------------------------
# checks shared by the entry points

def _check_g16(g16, ref, inp, c, what, key, enforce_global=True):
    """a 16-bit q|k|v gradient with the rotation undone against the reference: elements, then the global bar"""
    nq, nkv, T, dt = inp.nq, inp.nkv, inp.T, inp.dt
    want = _unrotate(ref.g, inp.cos, inp.sin, nq + nkv, T)
    unit, rest = ref.bound_parts(dt, c)
    zero = torch.zeros_like(ref.g)
    unit_r = _rot_bound(unit, zero, inp.cos, inp.sin, nq + nkv, T)
    rest_r = _rot_bound(rest + zero, ref.g, inp.cos, inp.sin, nq + nkv, T) + _ulp(want, dt)
    _check_elements(g16, want, unit_r, rest_r, c, what, key)
    if enforce_global:
        emul = _rnd(_unrotate(ref.g_emul, inp.cos, inp.sin, nq + nkv, T), dt)
        _check_global(g16, want, emul, nq, nkv, what, key)


def _check_g32(g32, ref, inp, c, what, key):
    unit, rest = ref.bound_parts(inp.dt, c)
    _check_elements(g32, ref.g, unit, rest + 0 * ref.g, c, what, key)
    _check_global(g32, ref.g, ref.g_emul.float().double(), inp.nq, inp.nkv, what, key)


def _check_stats_lse(stats, ref, inp, what):
    """(lse, 1, dO . att, 0): lse bit-equal to the input, delta within 64 * 2^-24 * sum|dO att| of float64"""
    assert _same_bits(stats[:, 0], inp.lse), f"{what}: stats[:, 0] is not the lse passed in"
    assert bool((stats[:, 1] == 1).all()) and bool((stats[:, 3] == 0).all()), f"{what}: stats[:, 1] / [:, 3]"
    d = (stats[:, 2].double() - ref.delta.reshape(-1)).abs()
    bad = d > _F_DELTA * _E * ref.delta_abs.reshape(-1)
    assert not bool(bad.any()), f"{what}: delta off at row {_first_bad(bad)}: {d[_first_bad(bad)].item():.3e}"


def _check_empty_samples(g, inp, what):
    for b, n in enumerate(inp.kv):
        rows = g.view(inp.B, inp.T, -1)[b]
        if n == 0:
            assert bool((rows == 0).all()), f"{what}: the gradient of sample {b} (kv_len 0) is not zero"
        assert bool((rows[n:, inp.nq * 64:] == 0).all()), f"{what}: dK / dV rows behind kv_len of sample {b} are not zero"


def _check_planted(g, stats, inp, dv_want, delta_want, out_dt, what, two_sweep=False, rotated=False):
    """dQ = dK = 0; dV the exact sums (rounded once into a 16-bit output); bit-zero rows behind kv_len; exact stats.
    rotated: the dK rows went through the transposed rotation after the accumulators; the rotation of a bit-zero pair is
    0 * cos + 0 * sin and 0 * cos - 0 * sin in fp32, which IEEE arithmetic signs by the table entries (-0 where cos < 0 and,
    in the first half, sin < 0 too).  Those exact bits are required: what a +0 accumulator pair gives, and nothing else."""
    B, T, nq, nkv = inp.case[:4]
    assert torch.isfinite(g).all(), f"{what}: non-finite gradient (a leaked key gives exp(512))"
    nz = g[:, : (nq + nkv) * 64] != 0
    if bool(nz.any()):
        r, c = _first_bad(nz)
        raise AssertionError(f"{what}: {int(nz.sum())} non-zero dQ / dK elements; first: sample {r // T} row {r % T} column {c} "
                             f"(head {c // 64}): {g[r, c].item()}")
    want = dv_want.float().to(out_dt)
    bad = _bits(g[:, (nq + nkv) * 64:].contiguous()) != _bits(want.contiguous())
    if bool(bad.any()):
        r, c = _first_bad(bad)
        raise AssertionError(f"{what}: {int(bad.any(-1).sum())} dV rows differ; first: sample {r // T} key {r % T} kv_len "
                             f"{inp.kv[r // T]} head {c // 64} dim {c % 64}: got {g[r, (nq + nkv) * 64 + c].item()} want {want[r, c].item()}")
    zbits = torch.zeros(T, (2 * nkv) * 64, dtype=out_dt, device=g.device)
    if rotated:
        z = torch.zeros(T, nkv, 32, device=g.device)
        cs, sn = inp.cos[:, None, :], inp.sin[:, None, :]
        zbits[:, : nkv * 64] = torch.cat([z * cs + z * sn, z * cs - z * sn], -1).reshape(T, nkv * 64).to(out_dt)
    for b, n in enumerate(inp.kv):
        tail = g.view(B, T, -1)[b, n:, nq * 64:]
        assert _same_bits(tail, zbits[n:]), f"{what}: dK / dV rows behind kv_len of sample {b} are not bit-zero"
    if stats is not None:
        has = (inp.tgt >= 0).permute(0, 2, 1).reshape(-1)
        zero = torch.zeros((), device=g.device)
        exp = torch.stack([torch.where(has, 512.0, 0.0), torch.where(has | (not two_sweep), 1.0, 0.0),
                           torch.where(has, delta_want.reshape(-1).float(), zero), torch.zeros_like(has, dtype=F32)], 1)
        if two_sweep:  # a query without a key: maximum -1e30, 1 / sum = 0
            exp[:, 0] = torch.where(has, exp[:, 0], torch.full_like(exp[:, 0], -1e30))
        bad = stats != exp
        assert not bool(bad.any()), f"{what}: stats differ at {_first_bad(bad)}: {stats[_first_bad(bad)[0]].tolist()} want {exp[_first_bad(bad)[0]].tolist()}"


_REFS = {}


def _real_case(case, dt, dev, with_lse=True):
    """realistic inputs and their reference, computed once per (case, type, form) and shared unchanged"""
    key = (_case_id(case), tuple(case[4]), dt, with_lse)
    if key not in _REFS:
        ikey = (_case_id(case), tuple(case[4]), dt, "inputs")
        if ikey not in _REFS:
            _REFS[ikey] = _realistic(case, dt, dev)
        _REFS[key] = (_REFS[ikey], Ref(_REFS[ikey], with_lse, dt))
    return _REFS[key]


# ---------------------------------------------------------------------------------------------------------------------------
# the formula against autograd

@pytest.mark.parametrize("case", RESIDENT_CASES + LONG_CASES + [TILED_CASES[0], TILED_CASES[2], TILED_CASES[3]], ids=_case_id)
def test_formula_matches_autograd(gpu, case):
    """float64 autograd of softmax(S) v against the formula with unrounded att and lse: 1e-12 relative per block"""
    dev = gpu["device"]
    B, T, nq, nkv, kv = case
    inp = _realistic(case, F16, dev)
    x = inp.qkv.double().clone().requires_grad_(True)
    v4 = x.view(B, T, nq + 2 * nkv, 64)
    g = nq // nkv
    q = v4[:, :, :nq].permute(0, 2, 1, 3)
    k = v4[:, :, nq:nq + nkv].permute(0, 2, 1, 3).repeat_interleave(g, dim=1)
    v = v4[:, :, nq + nkv:].permute(0, 2, 1, 3).repeat_interleave(g, dim=1)
    m = _mask(inp.kv_len, T)
    s = ((q @ k.transpose(-1, -2)) * SCALE).masked_fill(~m, float("-inf"))
    has = m.any(-1, keepdim=True)
    zero = torch.zeros((), dtype=F64, device=dev)
    p = torch.where(has, torch.softmax(torch.where(has, s, zero), -1), zero)  # a sample without keys: O = 0
    o = _flat(p @ v, B, T)
    o.backward(inp.dO.double())

    class Exact:  # the same inputs with unrounded statistics
        pass

    ex = Exact()
    ex.__dict__.update(inp.__dict__)
    ex.lse, ex.att = inp.lse64.reshape(-1), _flat(inp.o64, B, T)
    for with_lse in (True, False):
        ref = Ref(ex, with_lse, F16)
        for name, lo, hi in _blocks(nq, nkv):
            a, r = x.grad[:, lo:hi], ref.g[:, lo:hi]
            # (relative to max(norm, 1): at T = 1 the dq and dk blocks are zero up to the last bit of dP - delta)
            assert (a - r).norm().item() <= 1e-12 * max(a.norm().item(), 1.0), (name, with_lse, (a - r).norm().item(), a.norm().item())


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_attn_bwd_resident / tcavt_attn_bwd_long

def _two_launch_cases():
    return [("resident", c) for c in RESIDENT_CASES] + [("long", c) for c in LONG_CASES]


def _tl_key(entry, case, dt):
    return (f"tcavt_attn_bwd_{entry}", " + ".join(_paths(entry, case[1], case[2], case[3])), _name(dt))


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("entry,case", _two_launch_cases(), ids=lambda v: v if isinstance(v, str) else _case_id(v))
def test_two_launch_planted(gpu, entry, case, dt):
    dev = gpu["device"]
    ci = ALL_CASES.index(case)
    what = f"planted {entry} {_name(dt)}: {case}"
    inp, dv_want, delta = _planted(case, ci, dt, dev)
    g, stats = _two_launch(entry, inp, what)
    _check_planted(g, stats, inp, dv_want, delta, dt, what, rotated=True)
    # the float64 formula agrees with the construction (every other probability < e^-192)
    ref = Ref(inp, True, dt)
    assert (ref.g[:, : (inp.nq + inp.nkv) * 64].abs().max().item() < 1e-60
            and (ref.g[:, (inp.nq + inp.nkv) * 64:] - dv_want).abs().max().item() < 1e-60), "the planted construction is not exact"


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("entry,case", _two_launch_cases(), ids=lambda v: v if isinstance(v, str) else _case_id(v))
def test_two_launch_realistic(gpu, entry, case, dt):
    dev = gpu["device"]
    key = _tl_key(entry, case, dt)
    what = f"real {entry} {_name(dt)}: {case}"
    inp, ref = _real_case(case, dt, dev)
    g, stats = _two_launch(entry, inp, what)
    _check_stats_lse(stats, ref, inp, what)
    _check_empty_samples(g, inp, what)
    _check_g16(g, ref, inp, _C, what, key)
    g2, stats2 = _two_launch(entry, inp, what + " (second launch, zero rows behind the inputs)", fill=0.0)
    assert _same_bits(g2, g) and _same_bits(stats2, stats), f"{what}: two launches differ"
    if entry == "long" and _paths("resident", case[1], case[2], case[3]):
        _, stats_res = _two_launch("resident", inp, what + " (resident form)")
        assert _same_bits(stats_res, stats), f"{what}: stats differ from the resident form's"


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("entry,case", ADVERSARY_CASES, ids=lambda v: v if isinstance(v, str) else _case_id(v))
def test_adversaries(gpu, entry, case, dt):
    """score patterns that stress exp(S - lse) and the cancellation in dP - delta, under the bounds of the realistic regime"""
    dev = gpu["device"]
    for kind in ("increasing", "decreasing", "spike", "zero_q"):
        key = _tl_key(entry, case, dt)
        key = (key[0], key[1] + " adversary", key[2])
        what = f"{kind} {entry} {_name(dt)}: {case}"
        inp = _adversary(kind, case, dt, dev)
        ref = Ref(inp, True, dt)
        if kind == "zero_q":  # uniform P: lse = log(number of attended keys)
            nat = _mask(inp.kv_len, inp.T)[:, 0].sum(-1).double()
            assert bool(((inp.lse64 - torch.log(nat)[:, None, :]).abs() < 1e-12).all())
        g, stats = _two_launch(entry, inp, what)
        _check_stats_lse(stats, ref, inp, what)
        _check_g16(g, ref, inp, _C, what, key)


# ---------------------------------------------------------------------------------------------------------------------------
# the tiled form: tcavt_attn_bwd_scores + tcavt_attn_bwd_dkv + tcavt_rope_bwd_pack

def _tiled_key(case, with_lse, dt):
    ks = _paths("scores", case[1], case[2], case[3], with_lse, ("dQ", "stats")) + _paths("dkv", case[1], case[2], case[3])
    return ("tcavt_attn_bwd_scores + _dkv", " + ".join(ks), _name(dt))


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("with_lse", [True, False], ids=["lse", "two-sweep"])
@pytest.mark.parametrize("case", TILED_CASES, ids=_case_id)
def test_tiled_planted(gpu, case, with_lse, dt):
    dev = gpu["device"]
    ci = ALL_CASES.index(case)
    what = f"planted tiled {'lse' if with_lse else 'two-sweep'} {_name(dt)}: {case}"
    inp, dv_want, delta = _planted(case, ci, dt, dev)
    g32, stats, g16 = _tiled(inp, with_lse, what, "big")
    _check_planted(g32, stats, inp, dv_want, delta, F32, what, two_sweep=not with_lse)
    _check_planted(g16, None, inp, dv_want, delta, dt, what + " packed", rotated=True)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("with_lse", [True, False], ids=["lse", "two-sweep"])
@pytest.mark.parametrize("case", TILED_CASES, ids=_case_id)
def test_tiled_realistic(gpu, case, with_lse, dt):
    dev = gpu["device"]
    key = _tiled_key(case, with_lse, dt)
    what = f"real tiled {'lse' if with_lse else 'two-sweep'} {_name(dt)}: {case}"
    inp, ref = _real_case(case, dt, dev, with_lse)
    g32, stats, g16 = _tiled(inp, with_lse, what, "big")
    g32z, statsz, g16z = _tiled(inp, with_lse, what + " (zero pad rows)", 0.0)
    assert _same_bits(g32, g32z) and _same_bits(stats, statsz) and _same_bits(g16, g16z), f"{what}: the pad rows change the result"
    if with_lse:
        _check_stats_lse(stats, ref, inp, what)
    else:  # (maximum, 1 / sum, sum P dP, 0): the kernel's own statistics, checked through dK and dV below
        assert bool((stats[:, 3] == 0).all()), f"{what}: stats[:, 3]"
    _check_empty_samples(g32, inp, what)
    _check_g32(g32, ref, inp, _C, what, key)
    # the pack on top: the fp32 gradient rotated and rounded once
    want = _unrotate(g32.double(), inp.cos, inp.sin, inp.nq + inp.nkv, inp.T)
    _check_pack(g16, want, g32.double(), inp.cos, inp.sin, inp.nq + inp.nkv, inp.T, inp.dt, what + " pack", "rope_bwd_pack_kernel")
    _check_g16(g16, ref, inp, _C, what + " packed", (key[0] + " + tcavt_rope_bwd_pack", key[1], key[2]))


def _check_pack(out, want, src, cos, sin, n_rot_heads, L, dt, what, kernel):
    """a pack kernel's output against float64 of the transposed rotation: a few fp32 ulps of |a cos| + |b sin| (two products,
    one sum: 3 * 2^-24, bar 4) plus the output rounding (half an ulp of the type, bar one)"""
    z = torch.zeros_like(src)
    bnd = _rot_bound(z, src, cos, sin, n_rot_heads, L) * 2.0 + _ulp(want, dt)  # 4 * 2^-24 (|a cos| + |b sin|) + ulp_out
    d = (out.double() - want).abs()
    assert torch.isfinite(out).all(), f"{what}: non-finite (unwritten) elements"
    bad = d > bnd
    _record(("pack", kernel, _name(dt)), frac=(d / bnd).max().item())
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements out of bound, first {_first_bad(bad)}"


# ---------------------------------------------------------------------------------------------------------------------------
# the scores + gemm form (P^T, dS^T, dS of tcavt_attn_bwd_scores) and the two softmax-backward kernels

def _check_tiles(dS, PT, dST, ref, inp, what, key, eP, eS):
    """dS [B nq T, Tp], PT / dST [B nq Tp, Tp] against float64: one rounding plus the fp32 error; exact zeros where masked"""
    B, T, nq = inp.B, inp.T, inp.nq
    Tp = (T + 63) & ~63
    dt = dS.dtype
    u = _U[dt]
    sub = 2.0 ** -25 if dt == F16 else 0.0
    m = ref.m.expand(B, nq, T, T)
    gS = dS.view(B, nq, T, Tp)
    gPT = PT.view(B, nq, Tp, Tp)
    gST = dST.view(B, nq, Tp, Tp)
    assert bool((_bits(gS[..., T:].contiguous()) == 0).all()) and bool((_bits(gPT[:, :, T:].contiguous()) == 0).all())
    assert bool((_bits(gPT[..., T:].contiguous()) == 0).all()) and bool((_bits(gST[:, :, T:].contiguous()) == 0).all())
    assert bool((_bits(gST[..., T:].contiguous()) == 0).all())
    for got, want, err, nm in ((gS[..., :T], ref.dS, eS, "dS"), (gPT[:, :, :T, :T].transpose(-1, -2), ref.P, eP, "P^T"),
                               (gST[:, :, :T, :T].transpose(-1, -2), ref.dS, eS, "dS^T")):
        assert bool((_bits(got.contiguous())[~m] == 0).all()), f"{what}: {nm} is not bit-zero above the diagonal / behind kv_len"
        d = (got.double() - want).abs()
        unit = u * want.abs()
        rest = 1.01 * err + sub
        pos = m & (unit > 0)
        worst = max(((d - rest)[pos] / unit[pos]).max().item(), 0.0) if bool(pos.any()) else 0.0
        _record((key[0], key[1] + " " + nm, key[2]), c=worst)
        print(f"c {what} {nm}: {worst:.3f}")
        bad = d > _C * unit + rest
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements of {nm} out of bound (worst c {worst:.3f}), first {_first_bad(bad)}"


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("with_lse", [True, False], ids=["lse", "two-sweep"])
@pytest.mark.parametrize("case", TILED_CASES, ids=_case_id)
def test_scores_gemm_form(gpu, case, with_lse, dt):
    """tcavt_attn_bwd_scores with PT / dST / dS: each one rounding of the float64 P / dS plus the fp32 term; dQ under the
    bound of the other forms; dS^T the exact transpose of dS"""
    dev = gpu["device"]
    B, T, nq, nkv, kv = case
    inp = _real_case(case, dt, dev, with_lse)[0]
    ref = Ref(inp, with_lse, dt, keep_tiles=True)
    kname = _paths("scores", T, nq, nkv, with_lse, ("dQ", "dS", "PT"))[0]
    key = ("tcavt_attn_bwd_scores (PT / dST / dS)", kname, _name(dt))
    what = f"scores+gemm {'lse' if with_lse else 'two-sweep'} {_name(dt)}: {case}"
    dq, dS, PT, dST = _scores_gemm(inp, with_lse, what)
    _check_tiles(dS, PT, dST, ref, inp, what, key, ref.E_P, ref.E_S)
    Tp = (T + 63) & ~63
    assert _same_bits(dST.view(B, nq, Tp, Tp)[:, :, :T, :T].transpose(-1, -2), dS.view(B, nq, T, Tp)[..., :T]), f"{what}: dS^T is not dS transposed"
    unit, rest = ref.bound_parts(dt, _C)
    _check_elements(dq, ref.g[:, :nq * 64], unit[:, :nq * 64], rest[:, :nq * 64], _C, what + " dQ", key)


@pytest.mark.parametrize("form", ["tiles", "rows"])
@pytest.mark.parametrize("case", SOFTMAX_CASES, ids=_case_id)
def test_causal_softmax_bwd(gpu, case, form):
    """tcavt_causal_softmax_bwd_tiles / _rows (bf16) from fp32 S and dP: P = softmax(S), dS = scale P (dP - sum P dP) against
    float64 of the same fp32 inputs.  fp32 error: the row maximum is exact, the row sum and sum P dP are T additions, __expf is
    2 ulps after an argument error of 2^-24 |S - max|: eps_P = 2^-24 (T + 2 |S - max| + 8),
    E_S = eps_P |dS| + 2^-24 scale P ((T + 8) sum_j P |dP| + 4 (|dP| + |dot|))"""
    capi = _lib()
    dev = gpu["device"]
    B, T, nq, nkv, kv = case
    Tp = (T + 63) & ~63
    inp = _real_case(case, BF16, dev, False)[0]
    q, k, v, do = _heads(inp.qkv, inp.dO, B, T, nq, nkv)
    rows = B * nq * T
    S = torch.full((rows + 1, Tp), float("nan"), device=dev)  # columns >= T and the row behind are not the kernel's to use
    dP = torch.full((rows + 1, Tp), float("nan"), device=dev)
    S[:rows, :T] = ((q @ k.transpose(-1, -2)) * SCALE).float().view(rows, T)
    dP[:rows, :T] = (do @ v.transpose(-1, -2)).float().view(rows, T)
    keepS, keepD, keepL = S.clone(), dP.clone(), inp.kv_len.clone()
    m = _mask(inp.kv_len, T)

    class R:
        pass

    ref = R()
    s64, d64 = S[:rows, :T].double().view(B, nq, T, T), dP[:rows, :T].double().view(B, nq, T, T)
    zero = torch.zeros((), dtype=F64, device=dev)
    sm = s64.masked_fill(~m, float("-inf"))
    mx = torch.where(m.any(-1), sm.amax(-1), zero)
    lse = torch.where(m.any(-1), torch.logsumexp(sm, -1), zero)
    ref.P = torch.where(m, torch.exp(s64.masked_fill(~m, 0.0) - lse[..., None]), zero)
    dot = (ref.P * d64.masked_fill(~m, 0.0)).sum(-1)
    ref.dS = SCALE * ref.P * (d64.masked_fill(~m, 0.0) - dot[..., None])
    ref.m = m
    epsP = _E * (T + 2 * (s64 - mx[..., None]).abs().masked_fill(~m, 0.0) + 8)
    eP = epsP * ref.P
    eS = epsP * ref.dS.abs() + _E * SCALE * ref.P * ((T + 8) * (ref.P * d64.abs().masked_fill(~m, 0.0)).sum(-1)[..., None]
                                                      + 4 * (d64.abs().masked_fill(~m, 0.0) + dot.abs()[..., None]))
    what = f"causal_softmax_bwd_{form}: {case}"
    key = (f"tcavt_causal_softmax_bwd_{form}", _paths("softmax_" + form, T, nq, nkv)[0], "bf16")
    dS = Guarded(rows, Tp, BF16, dev, zero=True)
    if form == "tiles":
        PT = Guarded(B * nq * Tp, Tp, BF16, dev, zero=True)
        dST = Guarded(B * nq * Tp, Tp, BF16, dev, zero=True)
        rc = capi.lib().tcavt_causal_softmax_bwd_tiles(S.data_ptr(), dP.data_ptr(), dS.view.data_ptr(), PT.view.data_ptr(), dST.view.data_ptr(),
                                                       inp.kv_len.data_ptr(), B, T, Tp, nq, SCALE, capi.stream_ptr())
        torch.cuda.synchronize()
        capi.check(rc, what)
        assert dS.guards_ok() and PT.guards_ok() and dST.guards_ok(), f"{what}: write outside the outputs"
        _check_tiles(dS.view, PT.view, dST.view, ref, inp, what, key, eP, eS)
    else:
        P = Guarded(rows, Tp, BF16, dev)  # (this form writes every column: zero-filled by the kernel)
        dS = Guarded(rows, Tp, BF16, dev)
        rc = capi.lib().tcavt_causal_softmax_bwd_rows(S.data_ptr(), dP.data_ptr(), P.view.data_ptr(), dS.view.data_ptr(), inp.kv_len.data_ptr(),
                                                      B, T, Tp, nq, SCALE, capi.stream_ptr())
        torch.cuda.synchronize()
        capi.check(rc, what)
        assert dS.guards_ok() and P.guards_ok(), f"{what}: write outside the outputs"
        for got, want, err, nm in ((P.view, ref.P, eP, "P"), (dS.view, ref.dS, eS, "dS")):
            assert torch.isfinite(got).all(), f"{what}: non-finite (unwritten) {nm}"
            g4 = got.view(B, nq, T, Tp)
            assert bool((_bits(g4[..., T:].contiguous()) == 0).all()), f"{what}: {nm} columns behind T are not zero"
            mm = m.expand(B, nq, T, T)
            assert bool((_bits(g4[..., :T].contiguous())[~mm] == 0).all()), f"{what}: {nm} is not bit-zero where masked"
            d = (g4[..., :T].double() - want).abs()
            unit = _U[BF16] * want.abs()
            pos = mm & (unit > 0)
            worst = max(((d - 1.01 * err)[pos] / unit[pos]).max().item(), 0.0)
            _record((key[0], key[1] + " " + nm, "bf16"), c=worst)
            bad = d > _C * unit + 1.01 * err
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements of {nm} out of bound (worst c {worst:.3f})"
    assert _same_bits(S, keepS) and _same_bits(dP, keepD) and torch.equal(inp.kv_len, keepL), f"{what}: an input was modified"


# ---------------------------------------------------------------------------------------------------------------------------
# the scalar kernel

def _scalar(inp, what):
    capi = _lib()
    B, T, nq, nkv = inp.case[:4]
    bufs = inp.padded(3, float("nan"))
    snap = _snapshot(inp, bufs)
    g32 = Guarded(inp.M, inp.ncols, F32, inp.dev, zero=True)
    rc = capi.lib().tcavt_attn_causal_gqa_bwd(bufs[0].data_ptr(), bufs[1].data_ptr(), g32.view.data_ptr(), inp.kv_len.data_ptr(), B, T,
                                              nq, nkv, 64, SCALE, capi.stream_ptr())
    torch.cuda.synchronize()
    capi.check(rc, what)
    assert g32.guards_ok(), f"{what}: write outside g32"
    assert torch.isfinite(g32.view).all(), f"{what}: non-finite gradient"
    _unchanged(inp, bufs, snap, what)
    return g32.view


@pytest.mark.parametrize("case", SCALAR_CASES, ids=_case_id)
def test_scalar_kernel(gpu, case):
    """tcavt_attn_causal_gqa_bwd (bf16 inputs, fp32 arithmetic and output, float atomics): planted exactly, realistic under the
    bound with c = 0 (no 16-bit rounding on the path: the fp32 terms alone)"""
    dev = gpu["device"]
    ci = ALL_CASES.index(case)
    inp, dv_want, delta = _planted(case, ci, BF16, dev)
    _check_planted(_scalar(inp, f"planted scalar: {case}"), None, inp, dv_want, delta, F32, f"planted scalar: {case}")
    inp, ref = _real_case(case, BF16, dev, False)
    what = f"real scalar: {case}"
    g32 = _scalar(inp, what)
    _check_empty_samples(g32, inp, what)
    key = ("tcavt_attn_causal_gqa_bwd", "attn_causal_gqa_bwd_kernel", "bf16")
    unit, rest = ref.bound_parts(BF16, 0.0)
    _check_elements(g32, ref.g, unit, rest + 0 * ref.g, 0.0, what, key)
    _check_global(g32, ref.g, ref.g_emul, inp.nq, inp.nkv, what, key)


# ---------------------------------------------------------------------------------------------------------------------------
# the pack kernels on their own

@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_rope_bwd_pack(gpu, dt):
    """L = 37 (not a multiple of 16), 3 samples, 5 heads of which 3 rotate (rope_cols < ncols)"""
    from tcavt_amd.config import LlamaShape
    from tcavt_amd.rope import rope_tables

    capi = _lib()
    dev = gpu["device"]
    L, B, heads, rot = 37, 3, 5, 3
    M, ncols = B * L, heads * 64
    g = torch.Generator().manual_seed(5)
    src = (torch.randn(M, ncols, generator=g) * torch.exp(3 * torch.randn(M, 1, generator=g))).to(dev)
    cos, sin = (t.to(dev) for t in rope_tables(LlamaShape(), L))
    keep = (src.clone(), cos.clone(), sin.clone())
    out = Guarded(M, ncols, dt, dev)
    rc = capi.lib().tcavt_rope_bwd_pack(src.data_ptr(), out.view.data_ptr(), cos.data_ptr(), sin.data_ptr(), M, ncols, rot * 64, L,
                                        _dt_code(dt), capi.stream_ptr())
    torch.cuda.synchronize()
    capi.check(rc, "rope_bwd_pack")
    assert out.guards_ok(), "rope_bwd_pack: write outside out"
    want = _unrotate(src.double(), cos, sin, rot, L)
    _check_pack(out.view, want, src.double(), cos, sin, rot, L, dt, "rope_bwd_pack: L 37", "rope_bwd_pack_kernel")
    assert _same_bits(out.view[:, rot * 64:], src[:, rot * 64:].to(dt)), "rope_bwd_pack: the columns behind rope_cols are a plain conversion"
    assert all(_same_bits(a, b) for a, b in zip((src, cos, sin), keep)), "rope_bwd_pack: an input was modified"


@pytest.mark.parametrize("nq,nkv", [(6, 2), (4, 4), (16, 1)])
def test_gqa_rope_bwd_pack(gpu, nq, nkv):
    """G3 = dQ | dK per query head | dV per query head -> bf16 q|k|v gradient: group sums (fp32, in head order: (group - 1)
    additions, 2^-24 each on the sum of absolute values) and the transposed rotation; L = 37"""
    from tcavt_amd.config import LlamaShape
    from tcavt_amd.rope import rope_tables

    capi = _lib()
    dev = gpu["device"]
    L, B = 37, 2
    M, grp = B * L, nq // nkv
    g = torch.Generator().manual_seed(nq)
    G3 = torch.randn(M, 3 * nq * 64, generator=g).to(dev)
    cos, sin = (t.to(dev) for t in rope_tables(LlamaShape(), L))
    keep = G3.clone()
    out = Guarded(M, (nq + 2 * nkv) * 64, BF16, dev)
    rc = capi.lib().tcavt_gqa_rope_bwd_pack(G3.data_ptr(), out.view.data_ptr(), cos.data_ptr(), sin.data_ptr(), M, nq, nkv, 64, L,
                                            capi.stream_ptr())
    torch.cuda.synchronize()
    capi.check(rc, "gqa_rope_bwd_pack")
    assert out.guards_ok(), "gqa_rope_bwd_pack: write outside out"
    x = G3.double().view(M, 3, nkv, grp, 64)
    summed = torch.cat([G3.double()[:, : nq * 64], x[:, 1].sum(2).reshape(M, -1), x[:, 2].sum(2).reshape(M, -1)], 1)
    sabs = torch.cat([torch.zeros(M, nq * 64, dtype=F64, device=dev), x[:, 1].abs().sum(2).reshape(M, -1), x[:, 2].abs().sum(2).reshape(M, -1)], 1)
    want = _unrotate(summed, cos, sin, nq + nkv, L)
    bnd = _rot_bound(_E * (grp - 1) * sabs, summed, cos, sin, nq + nkv, L) * 2.0 + _ulp(want, BF16)
    d = (out.view.double() - want).abs()
    assert torch.isfinite(out.view).all()
    _record(("pack", "gqa_rope_bwd_pack_kernel", "bf16"), frac=(d / bnd).max().item())
    assert not bool((d > bnd).any()), f"gqa_rope_bwd_pack: {int((d > bnd).sum())} elements out of bound, first {_first_bad(d > bnd)}"
    assert _same_bits(G3, keep)


# ---------------------------------------------------------------------------------------------------------------------------
# refusals

def test_attn_bwd_refusals(gpu):
    """argument errors before any launch (non-zero status, tcavt_last_error names the entry point, outputs untouched), and the
    _ok predicates against _paths"""
    capi = _lib()
    L = capi.lib()
    dev = gpu["device"]

    def two_launch(entry, T, nq, nkv, head_dim=64, shift=0):
        B, aT = 1, min(T, 544)
        ncols = (nq + 2 * nkv) * 64
        qkv = torch.randn(B * aT * ncols + 64, device=dev).to(F16)
        dO, att = (torch.randn(B * aT * nq * 64 + 64, device=dev).to(F16) for _ in range(2))
        lse = torch.zeros(B * nq * aT, device=dev)
        g = torch.full((B * aT * ncols + 64,), 7.0, dtype=F16, device=dev)  # (7: a written NaN must not pass for untouched)
        st = torch.full((B * nq * aT * 4,), 7.0, device=dev)
        cs = torch.ones(aT * 32, device=dev)
        kv = torch.full((B,), aT, dtype=torch.int32, device=dev)
        rc = getattr(L, "tcavt_attn_bwd_" + entry)(qkv.data_ptr() + 2 * shift, dO.data_ptr(), att.data_ptr(), lse.data_ptr(), g.data_ptr(),
                                                   st.data_ptr(), cs.data_ptr(), cs.data_ptr(), kv.data_ptr(), B, T, nq, nkv, head_dim, SCALE,
                                                   capi.F16, capi.stream_ptr())
        torch.cuda.synchronize()
        return rc, bool((g == 7).all()) and bool((st == 7).all())

    def scores(T, Tp, nq=4, nkv=1, lse=False, att=False, head_dim=64):
        ncols = (nq + 2 * nkv) * 64
        qkv = torch.randn((T + 63) * ncols, device=dev).to(F16)
        dO, at = (torch.randn((T + 63) * nq * 64, device=dev).to(F16) for _ in range(2))
        ls = torch.zeros(nq * T, device=dev)
        dq = torch.full((T, nq * 64), 7.0, device=dev)
        st = torch.full((nq * T, 4), 7.0, device=dev)
        kv = torch.full((1,), T, dtype=torch.int32, device=dev)
        rc = L.tcavt_attn_bwd_scores(qkv.data_ptr(), dO.data_ptr(), None, None, None, dq.data_ptr(), nq * 64, st.data_ptr(), kv.data_ptr(), 1, T,
                                     Tp, nq, nkv, head_dim, SCALE, capi.F16, ls.data_ptr() if lse else None, at.data_ptr() if att else None,
                                     capi.stream_ptr())
        torch.cuda.synchronize()
        return rc, bool((dq == 7).all()) and bool((st == 7).all())

    for entry, T, nq, nkv in (("resident", 64, 4, 1), ("long", 300, 4, 1)):
        rc, clean = two_launch(entry, T, nq, nkv)
        assert rc == 0 and not clean  # the harness itself: a good call is accepted and writes
    rc, clean = scores(64, 64, lse=True, att=True)
    assert rc == 0 and not clean
    refused = [("T = 257 resident", "attn_bwd_resident", lambda: two_launch("resident", 257, 4, 1)),
               ("T = 545 long", "attn_bwd_long", lambda: two_launch("long", 545, 4, 1)),
               ("group 3 resident", "attn_bwd_resident", lambda: two_launch("resident", 64, 3, 1)),
               ("group 3 long", "attn_bwd_long", lambda: two_launch("long", 300, 3, 1)),
               ("head_dim 32 resident", "attn_bwd_resident", lambda: two_launch("resident", 64, 4, 1, head_dim=32)),
               ("head_dim 32 long", "attn_bwd_long", lambda: two_launch("long", 300, 4, 1, head_dim=32)),
               ("head_dim 32 scores", "attn_bwd_scores", lambda: scores(64, 64, head_dim=32)),
               ("misaligned resident", "attn_bwd_resident", lambda: two_launch("resident", 64, 4, 1, shift=1)),
               ("misaligned long", "attn_bwd_long", lambda: two_launch("long", 300, 4, 1, shift=1)),
               ("lse without att", "attn_bwd_scores", lambda: scores(64, 64, lse=True)),
               ("Tp = T (not rounded up)", "attn_bwd_scores", lambda: scores(100, 100)),
               ("Tp = 192 for T = 100", "attn_bwd_scores", lambda: scores(100, 192))]
    for name, entry, call in refused:
        L.tcavt_attn_causal_gqa_bwd(None, None, None, None, 1, 1, 1, 1, 64, SCALE, capi.stream_ptr())
        assert "attn_causal_gqa_bwd" in _last_error()
        rc, clean = call()
        assert rc != 0, f"{name}: accepted"
        assert entry in _last_error(), f"{name}: tcavt_last_error = {_last_error()!r}"
        assert clean, f"{name}: a refused call wrote"
    for T in (1, 256, 257, 544, 545):
        for group in (1, 2, 3, 4, 8, 16):
            assert bool(L.tcavt_attn_bwd_resident_ok(T, group, 1)) == (_paths("resident", T, group, 1) is not None), (T, group)
            # (the dispatch hands the chunked form only what the resident form does not serve: T > 256)
            assert bool(L.tcavt_attn_bwd_long_ok(T, group, 1)) == (_paths("long", T, group, 1) is not None and T > 256), (T, group)
            assert bool(L.tcavt_attn_bwd_resident_ok(T, 2 * group, 2)) == bool(L.tcavt_attn_bwd_resident_ok(T, group, 1))
    # no query heads: every predicate says no (pure host calls, a T inside each one's own range; nothing is launched)
    assert L.tcavt_attn_bwd_resident_ok(96, 0, 1) == 0
    assert L.tcavt_attn_bwd_long_ok(300, 0, 1) == 0
    assert L.tcavt_attn_bwd_stream_ok(600, 0, 1) == 0


def test_report_worst_ratio(gpu):
    """(runs last in file order) prints the worst ratios measured in this session per (entry point, kernel, type)"""
    for k in sorted(_WORST):
        w = _WORST[k]
        print(f"{k[0]:44s} {k[2]:5s} {k[1]:72s} " + "  ".join(f"worst {n} {w[n]:7.3f}" for n in ("c", "r", "frac") if n in w))
