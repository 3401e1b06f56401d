"""The forward attention kernels against float64 on every path: tcavt_attn_causal_gqa(_lse), tcavt_mha, tcavt_softmax_rows.

Every case calls the C entry point and checks it against float64 torch on the GPU, computed from the same 16-bit (or fp32)
inputs.  Outputs live inside larger NaN-filled buffers with guard rows: every in-range element must be finite, every guard
element keep its bits, every input stay bit-unchanged.

Causal GQA attention (attn_causal_gqa_kernel<512 | 1024, fp16 | bf16>).  _paths() mirrors the host rule of
tcavt_attn_causal_gqa_lse: 2 * group * 64 threads, the 512-thread instantiation for groups up to 4 and the 1024-thread one above,
Lp = L rounded up to 32, and per-wave LDS output tiles (store path "tile") while K, V^T and the tiles fit in 160 KiB - 256 B,
direct permlane32_swap stores ("direct") otherwise.  test_paths_coverage asserts from it that the case list reaches every
instantiation on both store paths.  Cases (B, L, nq, nkv, kv_len), each in fp16 and bf16 and in both regimes:

| case | group / threads | store path | why |
|---|---|---|---|
| (3, 1, 4, 1, [1, 1, 0]) | 4 / 512 | tile | L = 1; one block; a sample with no key |
| (3, 33, 2, 2, [33, 32, 1]) | 1 / 128 | tile | group 1; L % 32 = 1; kv_len on a tile edge |
| (3, 96, 6, 2, [96, 65, 0]) | 3 / 384 | tile | group 3; odd block count (self-paired middle block) |
| (3, 256, 8, 2, [256, 170, 31]) | 4 / 512 | tile | product shape; exactly NPRE blocks per wave |
| (2, 257, 4, 1, [257, 256]) | 4 / 512 | tile | first length that enters the late load_q loop |
| (2, 320, 8, 1, [320, 300]) | 8 / 1024 | tile | group 8; last tile-path length |
| (2, 352, 16, 2, [352, 33]) | 8 / 1024 | direct | group 8; direct-store path |
| (2, 480, 4, 1, [480, 479]) | 4 / 512 | tile | group 4; last tile-path length |
| (2, 511, 4, 1, [511, 481]) | 4 / 512 | direct | group 4; direct path; L % 32 = 31 |
| (2, 544, 8, 2, [544, 513]) | 4 / 512 | direct | maximum length; 17 blocks |
| (1, 544, 2, 2, [544]) | 1 / 128 | tile | group 1 at maximum length (longest staging remainder loops) |
| (1, 544, 3, 1, [530]) | 3 / 384 | direct | group 3; direct path |
| (1, 544, 8, 1, [544]) | 8 / 1024 | direct | group 8 at maximum length |

Two input regimes:

- planted (bit-exact): per kv head the K rows are 8 * h_j, h_j random +-1 codes of length 64; query i of a head is 8 * h_t(i) with
  t(i) <= i' = min(i, kv_len - 1).  With scale 0.125 the target's score is 512 and every other key's is 8 * dot <= 320 (the setup
  asserts dot <= 40 on the CPU), 277 below it in the exponent's base-2 units: every other probability underflows to exactly 0 in
  fp32 and the output must equal V[t(i)] bit for bit (V rows are multiples of 1/16 in [-4, 4] with j // 32 and j % 32 in
  columns 0 and 1: exact in both types and pairwise distinct).  Target patterns, a different one per query head and sample:
  the diagonal i', 0, the first key of the diagonal tile, the last key of the tile before it, uniform random in [0, i'].
  K rows j >= kv_len hold 16 * h_m, double-weight copies of the targets the rows behind them ask for, and V rows j >= kv_len
  hold +-30000: a padding-mask leak changes the output instead of hiding in a zero.  lse must be within 8 fp32 ulps of 512.
- realistic: q, k ~ N(0, sigma^2), sigma in {0.5, 1, 2} by case, v ~ N(0, 1), padded rows filled as above (K rows j >= kv_len
  are 2 * a real row).  Per element
      |got - ref| <= c * 2^-11 * (P |V|)_id + 2^-25 * sum_{j attended} |V_jd| + ulp_out(ref)
  P the float64 softmax: fp16 rounding of P; P going subnormal in fp16 relative to a running maximum that later rises; the
  output rounding.  Worst case c <= 1 (+ < 0.02 from the fp32 score and exp2 errors); the bar is _C_P = 1.0.  Rows with one
  attended key hold V[0] bit for bit here too.  Globally rel_err(got, ref) <= r * rel_err(round_dt(ref), ref), the reference's
  own output-rounding floor: r = 2.0 (fp16), 1.25 (bf16); P at bf16 precision lands near 6 and 1.3.
  lse: |lse - logsumexp64| <= 16 ulp_f32(max(|lse|, 1)); exactly 0 (as out) for a sample with kv_len == 0.

test_attn_adversaries runs increasing / decreasing scores, a spike on the last allowed key and q = 0 under the same bound;
test_attn_refusals the argument checks.

tcavt_mha (mha_lds_kernel when the whole problem fits 60 KiB of LDS, mha_small_kernel otherwise; _whole() mirrors the rule) at
the product's shapes plus a pair that straddles the kernel choice, all nine in / out type pairs on that pair and the product's
pairs elsewhere, operands passed as column slices of q|k|v and k|v buffers, out inside a NaN-guarded wider buffer:
      |got - ref| <= c * 2^-24 * (dh + Lk) * (1 + smax) * (P |V|)_id + ulp_out(ref),   smax = max_j scale * sum_d |q_id k_jd|
with c = _C_MHA = 2.  tcavt_softmax_rows: |got - ref| <= 8 * 2^-24 * ref + ulp_out(ref), zero padding exact.

Measured worst ratios are written next to the bars and in profiles/attention_fwd_bounds.txt; test_report_worst_ratio prints
this session's (pytest -s).
"""
import itertools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
SCALE = 0.125
# P-rounding bar: c in |got - ref| <= c * 2^-11 * (P|V|) + ...  Worst-case derivation: c <= 1.02.  Measured on an MI355X, worst
# over cases and adversaries per instantiation (threads, type, store path):
#   512 f16 tile 0.582, 512 f16 direct 0.510, 1024 f16 tile 0.547, 1024 f16 direct 0.474,
#   512 bf16 tile 0.471, 512 bf16 direct 0.545, 1024 bf16 tile 0.484, 1024 bf16 direct 0.545
# (P rounded through bf16 instead: 3.1 .. 5.9; a CPU emulation of the kernel's arithmetic gives 0.27 .. 0.55 and 2.8 .. 5.1).
# profiles/attention_fwd_bounds.txt has every case
_C_P = 1.0
# global bar: rel_err(got, ref) <= r * rel_err(round_dt(ref), ref).  Measured: fp16 1.04 .. 1.35 (512 tile 1.326, 512 direct 1.331,
# 1024 tile 1.040, 1024 direct 1.347; the high values are the sigma = 0.5 cases), bf16 <= 1.006 on all four
_R_GLOBAL = {F16: 2.0, BF16: 1.25}
# lse bar, in fp32 ulps of max(|lse|, 1).  Measured: <= 2.8 on every instantiation
_LSE_ULPS = 16
# mha accumulation bar (fp32 arithmetic; worst-case derivation c <= 2).  Measured: mha_lds_kernel 0.016, mha_small_kernel 0.006
_C_MHA = 2.0
_WORST_C, _WORST_R, _WORST_LSE, _WORST_MHA, _WORST_SM = {}, {}, {}, {}, {}


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


def _ulp(x, dt):
    """ulp of dt at |x| (float64 tensor), subnormal spacing below the normal range"""
    p, emin = {F16: (10, -14), BF16: (7, -126), F32: (23, -126)}[dt]
    _, e = torch.frexp(x)
    e = torch.where(x == 0, torch.full_like(e, emin + 1), e)
    return torch.ldexp(torch.ones_like(x), (e - 1).clamp_min(emin) - p)


def _last_error():
    msg = _lib().lib().tcavt_last_error()
    return msg.decode() if msg else ""


def _first_bad(bad):
    return tuple(bad.nonzero()[0].tolist())


# ---------------------------------------------------------------------------------------------------------------------------
# host-rule mirror and the case list

def _paths(L, nq, nkv):
    """tcavt_attn_causal_gqa_lse's launch: group, threads, launch-bound instantiation, padded length, store path"""
    group = nq // nkv
    Lp = (L + 31) & ~31
    lds = Lp * 128 + 64 * (Lp + 4) * 2  # K rows + V^T rows
    ot_bytes = 2 * group * 32 * 144
    tile = ((lds + 15) & ~15) + ot_bytes <= 160 * 1024 - 256
    return dict(group=group, threads=2 * group * 64, maxt=512 if 2 * group * 64 <= 512 else 1024, Lp=Lp,
                store="tile" if tile else "direct", nqb=Lp // 32)


ATTN_CASES = [  # (B, L, nq, nkv, kv_len)
    (3, 1, 4, 1, [1, 1, 0]),
    (3, 33, 2, 2, [33, 32, 1]),
    (3, 96, 6, 2, [96, 65, 0]),
    (3, 256, 8, 2, [256, 170, 31]),
    (2, 257, 4, 1, [257, 256]),
    (2, 320, 8, 1, [320, 300]),
    (2, 352, 16, 2, [352, 33]),
    (2, 480, 4, 1, [480, 479]),
    (2, 511, 4, 1, [511, 481]),
    (2, 544, 8, 2, [544, 513]),
    (1, 544, 2, 2, [544]),
    (1, 544, 3, 1, [530]),
    (1, 544, 8, 1, [544]),
]
ADVERSARY_CASES = [(1, 300, 4, 1, [300]), (1, 544, 8, 1, [530])]


def _case_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}x{c[3]}"


def _inst(case, dt):
    p = _paths(case[1], case[2], case[3])
    return f"{p['maxt']} {_name(dt)} {p['store']}"


def test_paths_coverage():
    """the case list reaches all four instantiations (each case runs in fp16 and bf16) on both store paths, groups 1, 3, 4
    and 8, and the lengths at which the host rule switches the store path"""
    seen, groups = {512: set(), 1024: set()}, set()
    for B, L, nq, nkv, kv in ATTN_CASES:
        assert 1 <= B <= 3 and 1 <= L <= 544 and len(kv) == B
        p = _paths(L, nq, nkv)
        seen[p["maxt"]].add(p["store"])
        groups.add(p["group"])
    assert seen[512] == {"tile", "direct"} and seen[1024] == {"tile", "direct"}, seen
    assert {1, 3, 4, 8} <= groups, groups
    by_group = {}
    for B, L, nq, nkv, kv in ATTN_CASES:
        by_group.setdefault(nq // nkv, set()).add(_paths(L, nq, nkv)["store"])
    assert by_group[4] == by_group[8] == by_group[3] == {"tile", "direct"} and by_group[1] == {"tile"}, by_group
    # where the rule switches (last tile-path length per group; groups 1 and 2 never leave it)
    for group, last in ((4, 480), (8, 320), (3, 512)):
        assert _paths(last, group, 1)["store"] == "tile" and _paths(last + 1, group, 1)["store"] == "direct", group
    assert _paths(544, 1, 1)["store"] == _paths(544, 2, 1)["store"] == "tile"
    # edges: L = 1, L % 32 of 1 and 31, an odd block count, exactly and more than NPRE = 4 blocks per wave
    Ls = [c[1] for c in ATTN_CASES]
    assert 1 in Ls and any(L % 32 == 1 for L in Ls) and any(L % 32 == 31 for L in Ls)
    assert any(_paths(c[1], c[2], c[3])["nqb"] % 2 == 1 and c[1] > 32 for c in ATTN_CASES)
    assert 256 in Ls and 257 in Ls and 544 in Ls
    for c in ADVERSARY_CASES:
        assert _paths(c[1], c[2], c[3])["maxt"] in (512, 1024)
    assert {_paths(c[1], c[2], c[3])["maxt"] for c in ADVERSARY_CASES} == {512, 1024}


# ---------------------------------------------------------------------------------------------------------------------------
# launching with poisoned buffers; the float64 reference

_GUARD = 3  # rows of NaN before and after out; 64 floats around lse


class Launch:
    """One tcavt_attn_causal_gqa(_lse) call on qkv [B * L, (nq + 2 nkv) * 64] with out and lse inside NaN-filled buffers."""

    def __init__(self, qkv, kv_len, B, L, nq, nkv, with_lse=True, entry="lse"):
        capi = _lib()
        dev, dt = qkv.device, qkv.dtype
        n, W = B * L, nq * 64
        self.ob = torch.full((n + 2 * _GUARD, W), float("nan"), dtype=dt, device=dev)
        self.lb = torch.full((B * nq * L + 128,), float("nan"), dtype=F32, device=dev)
        ob0, lb0 = self.ob.clone(), self.lb.clone()
        self.out = self.ob[_GUARD:_GUARD + n]
        self.lse = self.lb[64:64 + B * nq * L].view(B, nq, L)
        if entry == "plain":
            self.rc = capi.lib().tcavt_attn_causal_gqa(qkv.data_ptr(), self.out.data_ptr(), kv_len.data_ptr(), B, L, nq, nkv, SCALE,
                                                       _dt_code(dt), capi.stream_ptr())
        else:
            self.rc = capi.lib().tcavt_attn_causal_gqa_lse(qkv.data_ptr(), self.out.data_ptr(), self.lse.data_ptr() if with_lse else None,
                                                           kv_len.data_ptr(), B, L, nq, nkv, SCALE, _dt_code(dt), capi.stream_ptr())
        torch.cuda.synchronize()
        self.guards_ok = (torch.equal(_bits(self.ob[:_GUARD]), _bits(ob0[:_GUARD]))
                          and torch.equal(_bits(self.ob[_GUARD + n:]), _bits(ob0[_GUARD + n:]))
                          and torch.equal(_bits(self.lb[:64]), _bits(lb0[:64]))
                          and torch.equal(_bits(self.lb[64 + B * nq * L:]), _bits(lb0[64 + B * nq * L:])))
        self.lse_untouched = torch.equal(_bits(self.lb), _bits(lb0))
        self.out_untouched = torch.equal(_bits(self.ob), _bits(ob0))


def _with_guard_rows(x):
    """x [rows, W] at the front of a buffer with three NaN rows behind it (the kernel clamps its row indices to L - 1)"""
    buf = torch.full((x.shape[0] + 3, x.shape[1]), float("nan"), dtype=x.dtype, device=x.device)
    buf[: x.shape[0]] = x
    return buf


def _run_checked(qkv, kv_len, B, L, nq, nkv, what):
    """Runs the kernel with lse (twice), without lse and through tcavt_attn_causal_gqa; asserts guards, finiteness, unchanged
    inputs, run-to-run and with / without lse bit identity.  Returns (out [B * L, nq * 64], lse [B, nq, L])."""
    capi = _lib()
    buf = _with_guard_rows(qkv)
    keep, keep_kv = buf.clone(), kv_len.clone()
    a = Launch(buf, kv_len, B, L, nq, nkv)
    capi.check(a.rc, what)
    assert a.guards_ok, f"{what}: write outside out / lse"
    assert torch.isfinite(a.out).all(), f"{what}: {int((~torch.isfinite(a.out)).sum())} non-finite (unwritten) out elements"
    assert torch.isfinite(a.lse).all(), f"{what}: {int((~torch.isfinite(a.lse)).sum())} non-finite (unwritten) lse elements"
    b = Launch(buf, kv_len, B, L, nq, nkv)
    c = Launch(buf, kv_len, B, L, nq, nkv, with_lse=False)
    d = Launch(buf, kv_len, B, L, nq, nkv, entry="plain")
    for o, nm in ((b, "second launch"), (c, "lse == NULL"), (d, "tcavt_attn_causal_gqa")):
        capi.check(o.rc, f"{what} {nm}")
        assert o.guards_ok, f"{what} {nm}: write outside out / lse"
        assert torch.equal(_bits(o.out), _bits(a.out)), f"{what}: out of the {nm} call differs"
    assert torch.equal(_bits(b.lse), _bits(a.lse)), f"{what}: lse differs between two launches"
    assert c.lse_untouched and d.lse_untouched, f"{what}: lse written by a call without lse"
    assert torch.equal(_bits(buf), _bits(keep)) and torch.equal(kv_len, keep_kv), f"{what}: qkv / kv_len modified"
    return a.out, a.lse


def _attn_ref(qkv, kv_len, B, L, nq, nkv):
    """float64 causal AND key-valid attention from the 16-bit inputs: out, lse (0 for a query without a key), P |V| and the sum
    of |V| over the attended keys, the first and the last two as [B * L, nq * 64]; n attended [B, L]"""
    g = nq // nkv
    x = qkv.double().view(B, L, nq + 2 * nkv, 64)
    q = x[:, :, :nq].permute(0, 2, 1, 3)
    k = x[:, :, nq:nq + nkv].permute(0, 2, 1, 3).repeat_interleave(g, dim=1)
    v = x[:, :, nq + nkv:].permute(0, 2, 1, 3).repeat_interleave(g, dim=1)
    i = torch.arange(L, device=qkv.device)
    m = ((i[None, :] <= i[:, None])[None] & (i[None, None, :] < kv_len[:, None, None]))[:, None]  # [B, 1, L, L]
    s = ((q @ k.transpose(-1, -2)) * SCALE).masked_fill(~m, float("-inf"))
    has = m.any(-1)  # [B, 1, L]
    lse = torch.where(has, torch.logsumexp(s, -1), torch.zeros((), dtype=torch.float64, device=qkv.device))
    p = torch.where(m, torch.exp(s.masked_fill(~m, 0.0) - lse[..., None]), torch.zeros((), dtype=torch.float64, device=qkv.device))
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(B * L, nq * 64)
    nat = m[:, 0].sum(-1)
    return flat(p @ v), lse, flat(p @ v.abs()), flat(m.double().expand(B, nq, L, L) @ v.abs()), nat


def _check_bound(got, ref, pav, sav, dt, what, key):
    """the per-element bound of the realistic regime; records the worst c"""
    g = got.double()
    d = (g - ref).abs()
    slack = d - 2.0 ** -25 * sav - _ulp(ref, dt)
    unit = 2.0 ** -11 * pav
    bad = slack > _C_P * unit
    pos = unit > 0
    worst = max((slack[pos] / unit[pos]).max().item(), 0.0) if bool(pos.any()) else 0.0  # (0: within the other two terms)
    _WORST_C[key] = max(_WORST_C.get(key, -1.0), worst)
    print(f"c {what}: {worst:.3f}")
    if bool(bad.any()):
        i = _first_bad(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of bound (worst c {worst:.3f}); first {i}: got {g[i].item()!r} "
                             f"ref {ref[i].item()!r} allowed {(_C_P * unit + 2.0 ** -25 * sav + _ulp(ref, dt))[i].item():.3e}")


def _check_global(got, ref, dt, what, key, enforce=True):
    """rel_err against the reference's own output-rounding floor (asserted in the realistic regime, recorded elsewhere)"""
    rel = lambda a: ((a.double() - ref).norm() / ref.norm()).item()
    floor = rel(ref.float().to(dt))
    e = rel(got)
    if floor > 0:
        _WORST_R[key] = max(_WORST_R.get(key, 0.0), e / floor)
        print(f"r {what}: {e / floor:.3f}  (rel {e:.3e}, rounding floor {floor:.3e})")
    assert not enforce or e <= _R_GLOBAL[dt] * floor, f"{what}: rel {e:.3e} > {_R_GLOBAL[dt]} * output-rounding floor {floor:.3e}"


def _check_lse(lse, ref, what, key):
    d = (lse.double() - ref).abs()
    u = _ulp(ref.abs().clamp_min(1.0), F32)
    worst = (d / u).max().item()
    _WORST_LSE[key] = max(_WORST_LSE.get(key, 0.0), worst)
    print(f"lse {what}: {worst:.2f} ulp")
    bad = d > _LSE_ULPS * u
    assert not bool(bad.any()), f"{what}: lse off by {worst:.1f} ulp at {_first_bad(bad)}"


def _check_single_key_rows(got, qkv, nat, B, L, nq, nkv, what):
    """a row with one attended key holds V[0] of its kv head exactly"""
    g = nq // nkv
    v0 = qkv.view(B, L, nq + 2 * nkv, 64)[:, 0, nq + nkv:].repeat_interleave(g, dim=1)  # [B, nq, 64]
    want = v0[:, None].expand(B, L, nq, 64)
    one = (nat == 1)[:, :, None, None].expand(B, L, nq, 64)
    assert bool(one.any()) or int(nat.max()) == 0
    bad = (_bits(got.view(B, L, nq, 64)) != _bits(want.contiguous())) & one
    assert not bool(bad.any()), f"{what}: a row with one key is not V[0] bit for bit, first {_first_bad(bad)}"


def _check_empty_samples(got, lse, kv_len, B, L, nq, what):
    for b in range(B):
        if int(kv_len[b]) == 0:
            assert bool((got.view(B, L, nq * 64)[b] == 0).all()), f"{what}: out of sample {b} (kv_len 0) is not 0"
            assert bool((lse[b] == 0).all()), f"{what}: lse of sample {b} (kv_len 0) is not 0"


# ---------------------------------------------------------------------------------------------------------------------------
# inputs

def _codes(n, g):
    return (torch.randint(0, 2, (n, 64), generator=g) * 2 - 1).float()


def _planted(case, ci, dt, dev):
    """qkv (dt, on dev) and the targets t [B, L, nq] (-1: no key)"""
    B, L, nq, nkv, kv = case
    grp = nq // nkv
    g = torch.Generator().manual_seed(1000 + ci)
    x = torch.zeros(B, L, nq + 2 * nkv, 64)
    tgt = torch.full((B, L, nq), -1, dtype=torch.long)
    i = torch.arange(L)
    for b in range(B):
        n = kv[b]
        ip = i.clamp_max(n - 1)
        first = 32 * (ip // 32)
        pats = [ip, torch.zeros_like(ip), first, (first - 1).clamp_min(0)]
        for h in range(nkv):
            code = _codes(L, g)
            if n > 1:
                dots = code[:n] @ code[:n].T
                dots.fill_diagonal_(-64)
                assert dots.max().item() <= 40, f"planted codes too close: dot {dots.max().item()}"  # 8 * 40 = 320 << 512
            # padded K rows: double-weight copies of the targets that the rows behind them ask for
            src = torch.stack([p[-1] for p in pats])[i % 4] if n > 0 else i
            x[b, :, nq + h] = torch.where((i < n)[:, None], 8 * code, 16 * code[src])
            v = torch.randint(-64, 65, (L, 64), generator=g).float() / 16
            v[:, 0], v[:, 1] = (i // 32).float(), (i % 32).float()
            sign = (torch.randint(0, 2, (L, 64), generator=g) * 2 - 1).float()
            x[b, :, nq + nkv + h] = torch.where((i < n)[:, None], v, 30000.0 * sign)
            for hq in range(h * grp, (h + 1) * grp):
                if n == 0:
                    x[b, :, hq] = 8 * _codes(L, g)
                    continue
                rnd = (torch.rand(L, generator=g) * (ip + 1).float()).long().clamp_max(ip)
                t = (pats + [rnd])[(hq + b + ci) % 5]
                assert bool((t <= ip).all()) and bool((t >= 0).all())
                tgt[b, :, hq] = t
                x[b, :, hq] = 8 * code[t]
    qkv = x.view(B * L, -1).to(dt)
    assert torch.equal(qkv.float()[:, : (nq + nkv) * 64], x.view(B * L, -1)[:, : (nq + nkv) * 64])  # q and k exact in dt
    return qkv.to(dev), tgt.to(dev)


def _pad_rows(x, case, g):
    """rows j >= kv_len of the K and V blocks of x [B, L, nq + 2 nkv, 64]: K = 2 * a real row, V = +-30000"""
    B, L, nq, nkv, kv = case
    i = torch.arange(L)
    for b in range(B):
        n = kv[b]
        pad = (i >= n)[:, None, None]
        src = i % n if n > 0 else i
        x[b, :, nq:nq + nkv] = torch.where(pad, 2 * x[b, src, nq:nq + nkv], x[b, :, nq:nq + nkv])
        sign = (torch.randint(0, 2, (L, nkv, 64), generator=g) * 2 - 1).float()
        x[b, :, nq + nkv:] = torch.where(pad, 30000.0 * sign, x[b, :, nq + nkv:])
    return x


def _realistic(case, ci, dt, dev):
    B, L, nq, nkv, kv = case
    g = torch.Generator().manual_seed(2000 + ci)
    sigma = (0.5, 1.0, 2.0)[ci % 3]
    x = torch.randn(B, L, nq + 2 * nkv, 64, generator=g)
    x[:, :, : nq + nkv] *= sigma
    return _pad_rows(x, case, g).view(B * L, -1).to(dt).to(dev)


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_attn_causal_gqa(_lse)

@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("ci", range(len(ATTN_CASES)), ids=[_case_id(c) for c in ATTN_CASES])
def test_attn_planted(gpu, ci, dt):
    """out == V[t(i)] bit for bit; lse within 8 fp32 ulps of 512; a sample without a key gives exact zeros"""
    case = ATTN_CASES[ci]
    B, L, nq, nkv, kv = case
    dev = gpu["device"]
    what = f"planted {_inst(case, dt)}: {case}"
    qkv, tgt = _planted(case, ci, dt, dev)
    kv_len = torch.tensor(kv, dtype=torch.int32, device=dev)
    out, lse = _run_checked(qkv, kv_len, B, L, nq, nkv, what)
    x = qkv.view(B, L, nq + 2 * nkv, 64)
    vh = x[:, :, nq + nkv:].repeat_interleave(nq // nkv, dim=2)  # [B, L, nq, 64]
    want = torch.gather(vh, 1, tgt.clamp_min(0)[..., None].expand(B, L, nq, 64))
    want = torch.where((tgt >= 0)[..., None], want, torch.zeros((), dtype=dt, device=dev))
    bad = _bits(out.view(B, L, nq, 64)) != _bits(want.contiguous())
    if bool(bad.any()):
        b, i, h, d = _first_bad(bad)
        raise AssertionError(f"{what}: {int(bad.any(-1).sum())} rows are not V[target]; first: sample {b} query {i} head {h} target "
                             f"{int(tgt[b, i, h])} kv_len {kv[b]}: got key (tile, offset) = {out.view(B, L, nq, 64)[b, i, h, :2].tolist()} "
                             f"dim {d}: {out.view(B, L, nq, 64)[b, i, h, d].item()} != {want[b, i, h, d].item()}")
    # the float64 reference agrees with the construction (every other probability < 2^-277)
    ref, lse_ref, _, _, _ = _attn_ref(qkv, kv_len, B, L, nq, nkv)
    assert torch.equal(ref.float().to(dt), want.view(B * L, nq * 64)), "the planted construction is not exact in float64"
    has = (tgt >= 0).permute(0, 2, 1)  # [B, nq, L]
    exp_lse = torch.where(has, 512.0, 0.0).double()
    assert bool(((lse_ref - exp_lse).abs() < 1e-9).all())
    d = (lse.double() - exp_lse).abs()
    assert bool((d <= 8 * 2.0 ** -14).all()), f"{what}: lse off 512 by {d.max().item():.3e} (8 ulp = 4.9e-4)"
    _check_empty_samples(out, lse, kv, B, L, nq, what)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("ci", range(len(ATTN_CASES)), ids=[_case_id(c) for c in ATTN_CASES])
def test_attn_realistic(gpu, ci, dt):
    case = ATTN_CASES[ci]
    B, L, nq, nkv, kv = case
    dev = gpu["device"]
    key = _inst(case, dt)
    what = f"real {key}: {case}"
    qkv = _realistic(case, ci, dt, dev)
    kv_len = torch.tensor(kv, dtype=torch.int32, device=dev)
    out, lse = _run_checked(qkv, kv_len, B, L, nq, nkv, what)
    ref, lse_ref, pav, sav, nat = _attn_ref(qkv, kv_len, B, L, nq, nkv)
    _check_single_key_rows(out, qkv, nat, B, L, nq, nkv, what)
    _check_empty_samples(out, lse, kv, B, L, nq, what)
    _check_bound(out, ref, pav, sav, dt, what, key)
    _check_global(out, ref, dt, what, key)
    _check_lse(lse, lse_ref, what, key)


def _adversary(kind, case, dt, dev):
    B, L, nq, nkv, kv = case
    g = torch.Generator().manual_seed(L + len(kind))
    x = torch.randn(B, L, nq + 2 * nkv, 64, generator=g)
    u = torch.randn(64, generator=g)
    u = u / u.norm() * 8  # q . k = 64 ramp, scaled score 8 ramp
    j = torch.arange(L).float()
    if kind in ("increasing", "decreasing"):
        # scores move by 40 nats over the keys (1.2 .. 2.4 per tile): the running maximum rises in every tile, or the late
        # probabilities fall below 2^-24 of the first
        ramp = (j if kind == "increasing" else L - 1 - j) * (40.0 / (8 * L))
        x[:, :, :nq] = u + 0.05 * x[:, :, :nq]
        x[:, :, nq:nq + nkv] = ramp[None, :, None, None] * u + 0.05 * x[:, :, nq:nq + nkv]
    elif kind == "spike":
        # q_i = k_i (every head): the row's own key scores 0.125 |k_i|^2 ~ 18 +- 3, the others N(0, 2.25^2)
        x[:, :, nq:nq + nkv] *= 1.5
        x[:, :, :nq] = x[:, :, nq:nq + nkv].repeat_interleave(nq // nkv, dim=2)
    elif kind == "zero_q":
        x[:, :, :nq] = 0.0
    return _pad_rows(x, case, g).view(B * L, -1).to(dt).to(dev)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ADVERSARY_CASES, ids=_case_id)
def test_attn_adversaries(gpu, case, dt):
    """score patterns that stress the online softmax, under the bound of the realistic regime"""
    B, L, nq, nkv, kv = case
    dev = gpu["device"]
    kv_len = torch.tensor(kv, dtype=torch.int32, device=dev)
    for kind in ("increasing", "decreasing", "spike", "zero_q"):
        key = _inst(case, dt)
        what = f"{kind} {key}: {case}"
        qkv = _adversary(kind, case, dt, dev)
        out, lse = _run_checked(qkv, kv_len, B, L, nq, nkv, what)
        ref, lse_ref, pav, sav, nat = _attn_ref(qkv, kv_len, B, L, nq, nkv)
        if kind == "decreasing":
            x = qkv.double().view(B, L, nq + 2 * nkv, 64)
            s = SCALE * (x[0, L - 1, 0] @ x[0, :, nq].T)
            assert (s[0] - s[kv[0] - 1]).item() > 17.0  # past 2^-24: the last keys' P is below fp16's smallest subnormal
        if kind == "zero_q":
            assert bool(((lse_ref - torch.log(nat.double())[:, None, :]).abs() < 1e-12).all())  # uniform P: lse = log n
        _check_single_key_rows(out, qkv, nat, B, L, nq, nkv, what)
        _check_bound(out, ref, pav, sav, dt, what, key + " adversary")
        _check_global(out, ref, dt, what, key + " adversary", enforce=False)
        _check_lse(lse, lse_ref, what, key + " adversary")


def test_attn_refusals(gpu):
    """bad arguments: non-zero status, tcavt_last_error set, out untouched"""
    dev = gpu["device"]
    capi = _lib()

    def call(B, L, nq, nkv, dt_code=None, shift_qkv=0, shift_out=0, alloc_L=None):
        aL = max(alloc_L or L, 1)
        qkv = torch.randn(B * aL * (nq + 2 * nkv) * 64 + 8, device=dev).to(F16)
        ob = torch.full((B * aL * nq * 64 + 8 + 1024,), float("nan"), dtype=F16, device=dev)
        lb = torch.full((B * nq * aL + 64,), float("nan"), dtype=F32, device=dev)
        ob0, lb0 = ob.clone(), lb.clone()
        kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
        rc = capi.lib().tcavt_attn_causal_gqa_lse(qkv.data_ptr() + 2 * shift_qkv, ob.data_ptr() + 2 * shift_out, lb.data_ptr(),
                                                  kv_len.data_ptr(), B, L, nq, nkv, SCALE, capi.F16 if dt_code is None else dt_code,
                                                  capi.stream_ptr())
        torch.cuda.synchronize()
        return rc, torch.equal(_bits(ob), _bits(ob0)) and torch.equal(_bits(lb), _bits(lb0))

    rc, clean = call(2, 64, 4, 1)
    assert rc == 0 and not clean  # the harness itself: a good call is accepted and writes
    for name, kw in (("L = 0", dict(B=1, L=0, nq=4, nkv=1)), ("L = 545", dict(B=1, L=545, nq=4, nkv=1)),
                     ("group 9", dict(B=1, L=64, nq=9, nkv=1)), ("nq % nkv", dict(B=1, L=64, nq=5, nkv=2)),
                     ("f32", dict(B=1, L=64, nq=4, nkv=1, dt_code=capi.F32)),
                     ("unaligned qkv", dict(B=1, L=64, nq=4, nkv=1, shift_qkv=1)),
                     ("unaligned out", dict(B=1, L=64, nq=4, nkv=1, shift_out=1))):
        capi.lib().tcavt_attn_causal_gqa_lse(None, None, None, None, 1, 1, 1, 1, SCALE, capi.F16, capi.stream_ptr())
        assert "null pointer" in _last_error()
        rc, clean = call(**kw)
        assert rc != 0, f"{name}: accepted"
        assert "attn_causal_gqa" in _last_error() and "null pointer" not in _last_error(), f"{name}: tcavt_last_error = {_last_error()!r}"
        assert clean, f"{name}: a refused call wrote"


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_mha

def _whole(Lq, Lk, dh):
    """tcavt_mha's kernel choice: the whole (batch, head) problem in LDS (mha_lds_kernel) or the scores only (mha_small_kernel)"""
    return ((Lq + 2 * Lk) * (dh + 1) + Lq * Lk) * 4 <= 60 * 1024


MHA_SHAPES = [  # (Lq, Lk, nh, dh)
    (64, 64, 4, 16), (18, 18, 8, 96), (30, 30, 4, 32), (30, 256, 2, 1024), (64, 64, 2, 57), (64, 64, 2, 58), (16, 6, 8, 96),
    (1, 1, 1, 8),
]
MHA_ALL_PAIRS = [(64, 64, 2, 57), (64, 64, 2, 58)]
_PRODUCT_PAIRS = [(F32, F32), (F32, F16), (F32, BF16), (F16, F32), (BF16, F32)]


def test_mha_kernel_choice():
    assert ((64 + 128) * 58 + 64 * 64) * 4 == 60928 and _whole(64, 64, 57)
    assert ((64 + 128) * 59 + 64 * 64) * 4 == 61696 and not _whole(64, 64, 58)
    kinds = {s: _whole(s[0], s[1], s[3]) for s in MHA_SHAPES}
    assert kinds[(64, 64, 4, 16)] and kinds[(18, 18, 8, 96)] and kinds[(30, 30, 4, 32)] and kinds[(16, 6, 8, 96)] and kinds[(1, 1, 1, 8)]
    assert not kinds[(30, 256, 2, 1024)]
    assert {_whole(s[0], s[1], s[3]) for s in MHA_ALL_PAIRS} == {True, False}  # every type pair on both kernels


def _mha_ref(q, k, v, klen, B, Lq, Lk, nh, dh, scale):
    dev = q.device
    qh = q.double().reshape(B, Lq, nh, dh).transpose(1, 2)
    kh = k.double().reshape(B, Lk, nh, dh).transpose(1, 2)
    vh = v.double().reshape(B, Lk, nh, dh).transpose(1, 2)
    m = (torch.arange(Lk, device=dev)[None, :] < klen[:, None])[:, None, None, :]  # [B, 1, 1, Lk]
    s = ((qh @ kh.transpose(-1, -2)) * scale).masked_fill(~m, float("-inf"))
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    lse = torch.where(m.any(-1), torch.logsumexp(s, -1), zero)
    p = torch.where(m, torch.exp(s.masked_fill(~m, 0.0) - lse[..., None]), zero)
    smax = ((qh.abs() @ kh.abs().transpose(-1, -2)) * scale).masked_fill(~m, 0.0).amax(-1, keepdim=True)
    flat = lambda t: t.transpose(1, 2).reshape(B * Lq, nh * dh)
    return flat(p @ vh), flat((1 + smax) * (p @ vh.abs()))


@pytest.mark.parametrize("shape", MHA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mha(gpu, shape):
    from tcavt_amd import ops

    Lq, Lk, nh, dh = shape
    dev = gpu["device"]
    B, E = 3, nh * dh
    scale = torch.tensor(1.0 / math.sqrt(dh), dtype=F32).item()
    kernel = "mha_lds" if _whole(Lq, Lk, dh) else "mha_small"
    pairs = list(itertools.product((F32, BF16, F16), repeat=2)) if shape in MHA_ALL_PAIRS else _PRODUCT_PAIRS
    g = torch.Generator().manual_seed(Lq * 7 + Lk + dh)
    key_lens = [None, [Lk, Lk // 2, 1], [Lk + 7, 0, max(Lk - 1, 1)]]
    for in_dt in (F32, BF16, F16):
        if Lq == Lk:  # self-attention: q|k|v are column slices of one [rows, 3E] buffer
            X = torch.randn(B * Lq, 3 * E, generator=g).to(in_dt).to(dev)
            q, k, v = X[:, :E], X[:, E:2 * E], X[:, 2 * E:]
            srcs = [X]
        else:  # cross-attention: q of its own (padded rows), k|v slices of [rows, 2E]
            Q = torch.randn(B * Lq, E + 8, generator=g).to(in_dt).to(dev)
            KV = torch.randn(B * Lk, 2 * E, generator=g).to(in_dt).to(dev)
            q, k, v = Q[:, :E], KV[:, :E], KV[:, E:]
            srcs = [Q, KV]
        keep = [t.clone() for t in srcs]
        for kl in key_lens:
            key_len = None if kl is None else torch.tensor(kl, dtype=torch.int32, device=dev)
            klen = torch.full((B,), Lk, device=dev) if kl is None else key_len.clamp_max(Lk).long()
            ref, unit = _mha_ref(q, k, v, klen, B, Lq, Lk, nh, dh, scale)
            for out_dt in (o for i, o in pairs if i == in_dt):
                what = f"{kernel} {_name(in_dt)}->{_name(out_dt)} key_len={kl}: {shape}"
                buf = torch.full((B * Lq + 2, E + 16), float("nan"), dtype=out_dt, device=dev)
                before = buf.clone()
                out = buf[1:1 + B * Lq, 8:8 + E]
                ops.mha(q, k, v, out, B, Lq, Lk, nh, dh, scale, key_len=key_len)
                torch.cuda.synchronize()
                outside = torch.ones_like(buf, dtype=torch.bool)
                outside[1:1 + B * Lq, 8:8 + E] = False
                assert torch.equal(_bits(buf)[outside], _bits(before)[outside]), f"{what}: write outside out"
                got = out.double()
                assert torch.isfinite(got).all(), f"{what}: non-finite (unwritten) elements"
                d = (got - ref).abs()
                slack = d - _ulp(ref, out_dt)
                u = 2.0 ** -24 * (dh + Lk) * unit
                pos = u > 0
                if bool(pos.any()):
                    _WORST_MHA[kernel] = max(_WORST_MHA.get(kernel, -1.0), (slack[pos] / u[pos]).max().item())
                bad = slack > _C_MHA * u
                assert not bool(bad.any()), (f"{what}: {int(bad.sum())} out of bound, first {_first_bad(bad)}: got "
                                             f"{got[_first_bad(bad)].item()!r} ref {ref[_first_bad(bad)].item()!r}")
                if kl is not None:
                    for b in range(B):
                        if kl[b] == 0:
                            assert bool((out.reshape(B, Lq, E)[b] == 0).all()), f"{what}: key_len 0 must give exact zeros"
                        if min(kl[b], Lk) == 1:  # one key: P = 1, the row is V[0] rounded once
                            want = v.reshape(B, Lk, E)[b, 0].float().to(out_dt).expand(Lq, E)
                            assert torch.equal(out.reshape(B, Lq, E)[b], want), f"{what}: one key must give V[0]"
        for t, kp in zip(srcs, keep):
            assert torch.equal(_bits(t), _bits(kp)), "mha modified an input"


def test_mha_refusal(gpu):
    """Lq * Lk * 4 > 64 KiB: refused, out untouched"""
    dev = gpu["device"]
    capi = _lib()
    Lq, Lk, E = 128, 129, 8
    assert Lq * Lk * 4 > 64 * 1024 and Lq * (Lk - 1) * 4 <= 64 * 1024
    q, k, v = (torch.randn(n, E, device=dev) for n in (Lq, Lk, Lk))
    out = torch.full((Lq, E), float("nan"), device=dev)
    args = lambda lk: (q.data_ptr(), E, k.data_ptr(), E, v.data_ptr(), E, out.data_ptr(), E, None, 1, Lq, lk, 1, E, 0.35, capi.F32,
                       capi.F32, 0.0, 0, 0, capi.stream_ptr())
    rc = capi.lib().tcavt_mha(*args(Lk))
    torch.cuda.synchronize()
    assert rc != 0 and "mha" in _last_error() and bool(torch.isnan(out).all())
    capi.check(capi.lib().tcavt_mha(*args(Lk - 1)), "mha 128 x 128")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


# ---------------------------------------------------------------------------------------------------------------------------
# tcavt_softmax_rows

@pytest.mark.parametrize("out_dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("n_valid", [1, 100, 128])
def test_softmax_rows(gpu, n_valid, out_dt):
    from tcavt_amd import ops

    dev = gpu["device"]
    rows, n_out, lds, ldp = 37, 128, 144, 160
    g = torch.Generator().manual_seed(n_valid)
    s = torch.randn(rows, n_valid, generator=g) * 3
    s[3, n_valid // 2] += 60.0  # a spike: every other probability of the row ~ e^-60
    s[5] = 1.25  # equal values: P = 1 / n_valid
    S = torch.full((rows + 2, lds), float("nan"), device=dev)  # columns >= n_valid are not the kernel's to read
    S[:rows, :n_valid] = s.to(dev)
    P = torch.full((rows + 2, ldp), float("nan"), dtype=out_dt, device=dev)
    keep, before = S.clone(), P.clone()
    ops.softmax_rows(S, P, rows, n_valid, n_out, lds, ldp)
    torch.cuda.synchronize()
    what = f"softmax_rows n_valid={n_valid} {_name(out_dt)}"
    assert torch.equal(_bits(S), _bits(keep)), f"{what}: S modified"
    outside = torch.ones_like(P, dtype=torch.bool)
    outside[:rows, :n_out] = False
    assert torch.equal(_bits(P)[outside], _bits(before)[outside]), f"{what}: write outside P"
    assert bool((P[:rows, n_valid:n_out] == 0).all()), f"{what}: padding columns are not 0"
    ref = torch.softmax(S[:rows, :n_valid].double(), -1)
    got = P[:rows, :n_valid].double()
    assert torch.isfinite(got).all()
    d = (got - ref).abs()
    bad = d > 8 * 2.0 ** -24 * ref + _ulp(ref, out_dt)
    _WORST_SM[_name(out_dt)] = max(_WORST_SM.get(_name(out_dt), 0.0), (d / (8 * 2.0 ** -24 * ref + _ulp(ref, out_dt))).max().item())
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} out of bound, first {_first_bad(bad)}"
    if n_valid == 1:
        assert bool((got == 1).all())


def test_report_worst_ratio(gpu):
    """(runs last in file order) prints the worst ratios measured in this session, per instantiation and store path"""
    for k in sorted(_WORST_C):
        print(f"attn  {k:32s} worst c {_WORST_C[k]:7.3f}   worst r {_WORST_R.get(k, 0.0):6.3f}   lse {_WORST_LSE.get(k, 0.0):5.2f} ulp")
    for k in sorted(_WORST_MHA):
        print(f"mha   {k:32s} worst c {_WORST_MHA[k]:7.3f}")
    for k in sorted(_WORST_SM):
        print(f"softmax_rows {k:25s} worst |got - ref| / bound {_WORST_SM[k]:6.3f}")
