"""The decode attention kernel against float64 on every path: tcavt_attn_decode (attn_decode_kernel<fp16 | bf16, PFV>).

Every case calls the C entry point, in fp16 and bf16, and checks it against float64 torch on the GPU, computed from the same
16-bit inputs.  out and both caches live inside larger NaN-filled buffers with guard rows.  After every call: every guard
element keeps its bits; every cache row except pos[b] keeps its bits; cache row pos[b] holds the qkv row's k | v bits for
every kv head; qkv and pos are unchanged; every in-range out element is finite; for the fragment-major layouts 1 and 2 the token
slots >= B of out are unchanged and the un-permuted rows are bit-equal to layout 0 (layout 1 where B <= 32, layout 2 where
B <= 8); a second launch repeats the first bit for bit.

_paths() mirrors the host rule of tcavt_attn_decode and the kernel's split: KS = min(16, ceil(kv_lmax / 64)) waves per
(sample, query head), per sample n = pos[b] + 1 keys in chunks of chunk = ceil(ceil(n / KS) / 64) * 64 (64 up to n = 1024, 128
beyond: two rounds per wave), PFV (value-row prefetch) while B * nq <= 512.  test_paths_coverage asserts from it that the case
list reaches all four instantiations, KS in {1, 2, 3, 10, 16}, both chunk sizes, a wave with no key, a wave with exactly one
key and all three layouts.  Cases (B, nq, nkv, kv_lmax, pos), each in fp16 and bf16 and in both regimes:

| case | KS | PFV | what it reaches |
|---|---|---|---|
| (3, 4, 1, 48, [0, 20, 47]) | 1 | on | only the new key; last slot |
| (4, 4, 4, 100, [63, 64, 65, 99]) | 2 | on | group 1, round edge: second wave empty / 1 / 2 keys |
| (4, 8, 1, 130, [0, 64, 128, 129]) | 3 | on | group 8, third wave with 1 / 2 keys |
| (3, 8, 2, 640, [5, 575, 639]) | 10 | on | nine empty waves; stage-1 length |
| (4, 8, 2, 1024, [1023, 1022, 960, 511]) | 16 | on | chunk 64, every wave full |
| (4, 4, 1, 1088, [1024, 1087, 1025, 127]) | 16 | on | n = 1025: first length with chunk 128, ninth wave with one key |
| (3, 8, 2, 2048, [2047, 1500, 0]) | 16 | on | maximum length |
| (16, 32, 8, 100, ragged incl. 0, 63, 64, 99) | 2 | on | B * nq = 512: last PFV grid |
| (17, 32, 8, 100, ragged) | 2 | off | B * nq = 544: PFV off, 32-row fragment buffer |
| (33, 16, 2, 70, ragged) | 2 | off | group 8, PFV off, B > 32 (layout 0 only) |

Two input regimes:

- planted (bit-exact): per (sample, kv head) the keys are 8 * h_j, h_j random +-1 codes of length 64 (rows j < pos[b] in the cache,
  the new key in qkv); the query of a head is 8 * h_t.  With scale 0.125 the target's score is 512 and every other key's is
  8 * dot <= 320 (the setup asserts dot <= 40 on the CPU): every other probability underflows to exactly 0 in fp32, the sum is
  exactly 1 and out must equal V[t] bit for bit (V rows are multiples of 1/16 in [-4, 4] with j // 32 and j % 32 in columns 0 and
  1).  Target patterns, a different one per query head and sample: the new key pos[b] itself (k and v from qkv), key 0, keys 63
  and 64 (clamped to pos[b]), the first key of the last non-empty wave, the key before it, uniform random in [0, pos[b]].
  Cache row pos[b] (stale) and every row behind it hold 16 * h_target (the targets of the kv head's query heads in turn) in K
  and +-30000 in V: a read past pos[b], or of the stale row instead of qkv, changes the output instead of hiding in a zero.
- realistic: q, k ~ N(0, sigma^2), sigma in {0.5, 1, 2} by case, v ~ N(0, 1); the rows at and behind pos[b] hold 2 * a real key
  row and +-30000.  Per element
      |got - ref| <= c * 2^-11 * (P |V|)_d + 2^-25 * sum_{j attended} |V_jd| + ulp_out(ref)
  Derivation for this kernel: it forms p_j = fp16(exp(s_j - max) / sum) from fp32 scores, one global maximum and one global sum (no
  running maximum: a probability is rounded once, relative to the final sum), and accumulates p_j * V_jd in fp32.  fp16 rounding of
  a normal p_j is at most 2^-11 relative, of a subnormal one (p_j < 2^-14) at most 2^-25 absolute, the output rounding at most
  ulp_out(ref): c <= 1, plus the fp32 terms -- a score's error (64 fmas at |s| <= ~60: 2^-24 * 64 * |s| / 2, < 2^-12 absolute in the
  exponent), __expf (2 ulp) and the split-order sums over n <= 2048 (2^-24 * 11 levels) -- together under 0.05 of the first
  term.  The bar is _C_P = 1.0, as for the prefill kernels.  A row with n = 1 equals the new v bit for bit.  Globally
  rel_err(got, ref) <= r * rel_err(round_dt(ref), ref), r = 2.0 (fp16), 1.25 (bf16) as in test_attention_fwd_gpu.py.

test_adversaries runs increasing / decreasing scores (maximum in the last / first wave), a spike on the new key, q = 0 at
n = 2048 and equal large scores under the same per-element bound; test_refusals the argument checks (nothing is launched).

Measured worst ratios are written next to the bars and in profiles/attention_decode_bounds.txt; test_report_worst_ratio
prints this session's (pytest -s).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
SCALE = 0.125
# P-rounding bar: c in |got - ref| <= c * 2^-11 * (P|V|) + ...  (derivation above: c <= 1.05).  Measured on an MI355X, worst over
# the cases / over the adversaries per instantiation (type, value-row prefetch):
#   f16 pfv 0.585 / 0.206, f16 nopfv 0.690 / 0.645, bf16 pfv 0.448 / 0.111, bf16 nopfv 0.513 / 0.593
# (a float32 torch emulation of the kernel's arithmetic gives the same figures to three digits).
# profiles/attention_decode_bounds.txt has every case
_C_P = 1.0
# global bar: rel_err(got, ref) <= r * rel_err(round_dt(ref), ref).  Measured: f16 pfv 1.456, f16 nopfv 1.411 (adversaries, recorded
# only: 1.438 / 1.358), bf16 <= 1.011 on both
_R_GLOBAL = {F16: 2.0, BF16: 1.25}
_WORST_C, _WORST_R = {}, {}
_GUARD = 3  # NaN rows before and after out and the caches


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


def from_frag(f, Mr, C):
    """fragment-major [Mr * C] (blocks of 16 tokens, tcavt_pack_weight16 order) -> rows [Mr, C] (test_kernels_gpu.py)"""
    return f.view(Mr // 16, C // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(Mr, C)


def from_frag8(f, C):
    """ONE block of 8 tokens (TCAVT_ACT_BLOCK8) -> rows [8, C] (test_kernels_gpu.py)"""
    return f.view(C // 32, 4, 8, 8).permute(2, 0, 1, 3).reshape(8, C)


# ---------------------------------------------------------------------------------------------------------------------------
# host-rule mirror and the case list

def _paths(B, nq, kv_lmax, pos):
    """tcavt_attn_decode's launch and attn_decode_kernel's key split: KS, PFV, LDS bytes, and per sample n, chunk and the
    number of keys each of the KS waves holds"""
    KS = min(16, (kv_lmax + 63) // 64)
    lds = (kv_lmax + KS * 66) * 4
    per = []
    for p in pos:
        n = min(p + 1, kv_lmax)
        chunk = ((n + KS - 1) // KS + 63) // 64 * 64
        per.append(dict(n=n, chunk=chunk, keys=[max(0, min(chunk, n - k * chunk)) for k in range(KS)]))
    return dict(KS=KS, pfv=B * nq <= 512, lds=lds, per=per)


def _ragged(B, kv_lmax):
    """B positions that walk over the round edge: 0, 63, 64, kv_lmax - 1, then a stride that is no multiple of anything"""
    base = [0, 63, 64, kv_lmax - 1, 1, 62, 65]
    return [min(base[b], kv_lmax - 1) if b < len(base) else (b * 37 + 11) % kv_lmax for b in range(B)]


CASES = [  # (B, nq, nkv, kv_lmax, pos)
    (3, 4, 1, 48, [0, 20, 47]),
    (4, 4, 4, 100, [63, 64, 65, 99]),
    (4, 8, 1, 130, [0, 64, 128, 129]),
    (3, 8, 2, 640, [5, 575, 639]),
    (4, 8, 2, 1024, [1023, 1022, 960, 511]),
    (4, 4, 1, 1088, [1024, 1087, 1025, 127]),
    (3, 8, 2, 2048, [2047, 1500, 0]),
    (16, 32, 8, 100, _ragged(16, 100)),
    (17, 32, 8, 100, _ragged(17, 100)),
    (33, 16, 2, 70, _ragged(33, 70)),
]
ADVERSARY_CASES = [(2, 8, 1, 2048, [2047, 1029]), (17, 32, 8, 200, _ragged(17, 200))]


def _layouts(case):
    B, nq = case[0], case[1]
    return [0] + ([1] if B <= 32 and (nq * 64) % 256 == 0 else []) + ([2] if B <= 8 else [])


def _case_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}x{c[3]}"


def _inst(case, dt):
    return f"{_name(dt)} {'pfv' if _paths(case[0], case[1], case[3], case[4])['pfv'] else 'nopfv'}"


def test_paths_coverage():
    """the case list reaches all four instantiations (each case runs in fp16 and bf16), KS in {1, 2, 3, 10, 16}, both chunk
    sizes, a wave with no key, a wave with exactly one key, and all three layouts -- from the host rule alone"""
    ks, pfv, chunks, layouts, groups = set(), set(), set(), set(), set()
    empty = one = full = False
    for case in CASES + ADVERSARY_CASES:
        B, nq, nkv, lmax, pos = case
        assert len(pos) == B and all(0 <= p <= lmax - 1 for p in pos) and nq % nkv == 0
        p = _paths(B, nq, lmax, pos)
        assert p["lds"] <= 64 * 1024 and 1 <= p["KS"] <= 16
        for s in p["per"]:
            assert sum(s["keys"]) == s["n"], (case, s)  # the split covers every key once
    for case in CASES:
        B, nq, nkv, lmax, pos = case
        p = _paths(B, nq, lmax, pos)
        ks.add(p["KS"])
        pfv.add(p["pfv"])
        groups.add(nq // nkv)
        layouts.update(_layouts(case))
        for s in p["per"]:
            chunks.add(s["chunk"])
            empty |= 0 in s["keys"]
            one |= 1 in s["keys"] and p["KS"] > 1 and s["n"] > 1
            full |= p["KS"] == 16 and all(k == s["chunk"] for k in s["keys"])
    assert {1, 2, 3, 10, 16} <= ks, ks
    assert pfv == {True, False}
    assert chunks == {64, 128}, chunks
    assert empty and one and full
    assert layouts == {0, 1, 2}
    assert {1, 4, 8} <= groups, groups
    # where the rules switch: the last PFV grid and the first without; the last n with one round per wave and the first with two;
    # a 32-row fragment buffer; a case beyond the fragment-major layouts
    assert any(c[0] * c[1] == 512 for c in CASES) and any(c[0] * c[1] == 544 for c in CASES)
    ns = {s["n"] for c in CASES for s in _paths(c[0], c[1], c[3], c[4])["per"]}
    assert {1, 64, 65, 1024, 1025, 2048} <= ns, sorted(ns)
    assert any(16 < c[0] <= 32 and 1 in _layouts(c) for c in CASES) and any(c[0] > 32 for c in CASES)
    assert any(_layouts(c) == [0, 1, 2] for c in CASES)
    assert {_paths(c[0], c[1], c[3], c[4])["pfv"] for c in ADVERSARY_CASES} == {True, False}
    assert any(2048 in [s["n"] for s in _paths(c[0], c[1], c[3], c[4])["per"]] for c in ADVERSARY_CASES)


# ---------------------------------------------------------------------------------------------------------------------------
# launching with poisoned buffers; the float64 reference

def _guarded(x):
    """x [rows, W] between _GUARD NaN rows: (buffer, view of the middle)"""
    buf = torch.full((x.shape[0] + 2 * _GUARD, x.shape[1]), float("nan"), dtype=x.dtype, device=x.device)
    buf[_GUARD:_GUARD + x.shape[0]] = x
    return buf, buf[_GUARD:_GUARD + x.shape[0]]


def _launch(qkv, kc0, vc0, pos_t, case, layout, what):
    """One tcavt_attn_decode call on fresh copies of the caches; asserts every invariant that does not need the reference.
    Returns out [B, nq * 64] (un-permuted for layouts 1 and 2)."""
    capi = _lib()
    B, nq, nkv, lmax, pos = case
    dt, dev, W, w = qkv.dtype, qkv.device, nq * 64, nkv * 64
    what = f"{what} layout {layout}"
    kbuf, kc = _guarded(kc0.view(B * lmax, w))
    vbuf, vc = _guarded(vc0.view(B * lmax, w))
    qbuf, q = _guarded(qkv)
    rows = B if layout == 0 else 8 if layout == 2 else 16 * ((B + 15) // 16)
    obuf = torch.full((rows + 2 * _GUARD, W), float("nan"), dtype=dt, device=dev)
    out = obuf[_GUARD:_GUARD + rows]
    k0, v0, q0, o0, p0 = kbuf.clone(), vbuf.clone(), qbuf.clone(), obuf.clone(), pos_t.clone()
    rc = capi.lib().tcavt_attn_decode(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), pos_t.data_ptr(), out.data_ptr(), B, nq, nkv, lmax,
                                      SCALE, _dt_code(dt), layout, capi.stream_ptr())
    torch.cuda.synchronize()
    capi.check(rc, what)
    assert torch.equal(_bits(qbuf), _bits(q0)) and torch.equal(pos_t, p0), f"{what}: qkv / pos modified"
    for nm, buf, b0 in (("out", obuf, o0), ("k_cache", kbuf, k0), ("v_cache", vbuf, v0)):
        assert torch.equal(_bits(buf[:_GUARD]), _bits(b0[:_GUARD])) and torch.equal(_bits(buf[-_GUARD:]), _bits(b0[-_GUARD:])), \
            f"{what}: write into the guard rows of {nm}"
    # the caches: row pos[b] is the qkv row's k | v, every other row keeps its bits
    at = torch.zeros(B, lmax, dtype=torch.bool, device=dev)
    at[torch.arange(B, device=dev), pos_t.long()] = True
    at = at.view(B * lmax)
    for nm, c, c0, col in (("k_cache", kc, k0[_GUARD:-_GUARD], nq * 64), ("v_cache", vc, v0[_GUARD:-_GUARD], (nq + nkv) * 64)):
        same = (_bits(c) == _bits(c0)).all(-1)
        assert bool(same[~at].all()), f"{what}: {nm} row {_first_bad((~same & ~at).view(B, lmax))} (sample, row) was written"
        assert torch.equal(_bits(c[at]), _bits(qkv[:, col:col + w])), f"{what}: {nm} row pos[b] is not the qkv row's bits"
    if layout == 0:
        res = out
    else:
        full = from_frag(out.reshape(-1), rows, W) if layout == 1 else from_frag8(out.reshape(-1), W)
        assert torch.equal(_bits(full[B:]), _bits(torch.full_like(full[B:], float("nan")))), f"{what}: token slots >= B written"
        res = full[:B].contiguous()
    assert torch.isfinite(res).all(), f"{what}: {int((~torch.isfinite(res)).sum())} non-finite (unwritten) out elements"
    return res.clone()


def _run_checked(qkv, kc, vc, case, what):
    """layout 0 twice, then every other legal layout: bit-equal results.  Returns out [B, nq * 64]."""
    pos_t = torch.tensor(case[4], dtype=torch.int32, device=qkv.device)
    a = _launch(qkv, kc, vc, pos_t, case, 0, what)
    b = _launch(qkv, kc, vc, pos_t, case, 0, what + " (second launch)")
    assert torch.equal(_bits(a), _bits(b)), f"{what}: two launches differ"
    for layout in _layouts(case)[1:]:
        o = _launch(qkv, kc, vc, pos_t, case, layout, what)
        bad = _bits(o) != _bits(a)
        assert not bool(bad.any()), f"{what}: layout {layout} differs from layout 0 at (sample, column) {_first_bad(bad)}"
    return a


def _logical_kv(qkv, kc, vc, case):
    """K, V [B, nkv, lmax, 64] as the kernel must see them: the cache with row pos[b] taken from qkv"""
    B, nq, nkv, lmax, pos = case
    dev = qkv.device
    pos_t = torch.tensor(pos, device=dev)
    k = kc.view(B, lmax, nkv, 64).clone()
    v = vc.view(B, lmax, nkv, 64).clone()
    ar = torch.arange(B, device=dev)
    k[ar, pos_t] = qkv[:, nq * 64:(nq + nkv) * 64].view(B, nkv, 64)
    v[ar, pos_t] = qkv[:, (nq + nkv) * 64:].view(B, nkv, 64)
    return k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3), pos_t


def _ref(qkv, kc, vc, case):
    """float64 attention of the one query per (sample, head) over keys 0 .. pos[b]: out, P |V| and the sum of |V| over the
    attended keys, each [B, nq * 64]"""
    B, nq, nkv, lmax, pos = case
    g = nq // nkv
    k, v, pos_t = _logical_kv(qkv, kc, vc, case)
    k = k.double().repeat_interleave(g, dim=1)  # [B, nq, lmax, 64]
    v = v.double().repeat_interleave(g, dim=1)
    q = qkv[:, : nq * 64].double().view(B, nq, 1, 64)
    m = (torch.arange(lmax, device=qkv.device)[None, :] <= pos_t[:, None])[:, None, None, :]  # [B, 1, 1, lmax]
    zero = torch.zeros((), dtype=torch.float64, device=qkv.device)
    v = torch.where(m.transpose(-1, -2), v, zero)  # (the rows behind pos[b] hold +-30000: keep 0 * them out of the sums)
    s = ((q @ k.transpose(-1, -2)) * SCALE).masked_fill(~m, float("-inf"))
    p = torch.softmax(s, -1)
    flat = lambda t: t.reshape(B, nq * 64)
    return flat(p @ v), flat(p @ v.abs()), flat(m.double().expand(B, nq, 1, lmax) @ v.abs())


def _check_bound(got, ref, pav, sav, dt, what, key):
    """the per-element bound of the realistic regime; records the worst c"""
    g = got.double()
    d = (g - ref).abs()
    slack = d - 2.0 ** -25 * sav - _ulp(ref, dt)
    unit = 2.0 ** -11 * pav
    bad = slack > _C_P * unit
    nz = unit > 0
    worst = max((slack[nz] / unit[nz]).max().item(), 0.0) if bool(nz.any()) else 0.0  # (0: within the other two terms)
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


def _check_single_key_rows(got, qkv, case, what):
    """a sample with pos[b] == 0 attends the new key alone: its rows are the new v bit for bit"""
    B, nq, nkv, lmax, pos = case
    vnew = qkv[:, (nq + nkv) * 64:].view(B, nkv, 64).repeat_interleave(nq // nkv, dim=1).reshape(B, nq * 64)
    for b in range(B):
        if pos[b] == 0:
            assert torch.equal(_bits(got[b]), _bits(vnew[b])), f"{what}: sample {b} (one key) is not the new v bit for bit"


# ---------------------------------------------------------------------------------------------------------------------------
# inputs

def _signs(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def _patterns(n, chunk):
    """the planted targets of a sample with n keys split in `chunk`s: new key, 0, 63, 64, first key of the last non-empty
    wave, the key before it"""
    first = (n - 1) // chunk * chunk
    return [n - 1, 0, min(63, n - 1), min(64, n - 1), first, max(first - 1, 0)]


def _planted(case, ci, dt, dev):
    """qkv [B, (nq + 2 nkv) * 64], k_cache, v_cache [B, lmax, nkv * 64] (dt, on dev) and the targets [B, nq]"""
    B, nq, nkv, lmax, pos = case
    grp = nq // nkv
    g = torch.Generator().manual_seed(3000 + ci)
    per = _paths(B, nq, lmax, pos)["per"]
    code = _signs((B, nkv, lmax, 64), g)
    v = torch.randint(-64, 65, (B, nkv, lmax, 64), generator=g).float() / 16
    j = torch.arange(lmax)
    v[..., 0], v[..., 1] = (j // 32).float(), (j % 32).float()
    tgt = torch.zeros(B, nq, dtype=torch.long)
    for b in range(B):
        n = per[b]["n"]
        pats = _patterns(n, per[b]["chunk"])
        for hq in range(nq):
            which = (hq + b + ci) % (len(pats) + 1)
            tgt[b, hq] = pats[which] if which < len(pats) else int(torch.randint(0, n, (1,), generator=g))
    assert bool((tgt <= torch.tensor(pos)[:, None]).all()) and bool((tgt >= 0).all())
    kvh = torch.arange(nq) // grp
    qcode = code[torch.arange(B)[:, None], kvh[None, :], tgt]  # [B, nq, 64]
    # every non-target dot <= 40: the other keys score 8 * dot <= 320, 192 below the target's 512
    dots = torch.einsum("bhd,bhjd->bhj", qcode, code[:, kvh])  # [B, nq, lmax]
    other = (j[None, None, :] <= torch.tensor(pos)[:, None, None]) & (j[None, None, :] != tgt[..., None])
    assert dots[other].numel() == 0 or dots[other].max().item() <= 40, f"planted codes too close: dot {dots[other].max().item()}"
    # rows j >= pos[b] of the cache (the stale row pos[b] included): 16 * the code of a target of the kv head's query heads, in turn;
    # +-30000 in V
    behind = (j[None, :] >= torch.tensor(pos)[:, None])[:, None, :, None]  # [B, 1, lmax, 1]
    turn = (torch.arange(nkv)[:, None] * grp + j[None, :] % grp)  # [nkv, lmax]: query head whose target the row copies
    decoy = qcode[torch.arange(B)[:, None, None], turn[None]]  # [B, nkv, lmax, 64]
    kc = torch.where(behind, 16 * decoy, 8 * code)
    vc = torch.where(behind, 30000.0 * _signs((B, nkv, lmax, 64), g), v)
    ar = torch.arange(B)
    x = torch.cat([8 * qcode, 8 * code[ar, :, torch.tensor(pos)], v[ar, :, torch.tensor(pos)]], dim=1)  # [B, nq + 2 nkv, 64]
    want = v[torch.arange(B)[:, None], kvh[None, :], tgt]  # [B, nq, 64]
    qkv, kc, vc = x.view(B, -1).to(dt), kc.permute(0, 2, 1, 3).reshape(B, lmax, nkv * 64).to(dt), vc.permute(0, 2, 1, 3).reshape(B, lmax, nkv * 64).to(dt)
    assert torch.equal(qkv.float(), x.view(B, -1)) and torch.equal(want.to(dt).float(), want)  # exact in dt
    return qkv.to(dev), kc.contiguous().to(dev), vc.contiguous().to(dev), tgt, want.view(B, nq * 64).to(dt).to(dev)


def _with_decoys(x, kc, vc, case, g, dt, dev):
    """rows j >= pos[b] of kc / vc [B, lmax, nkv, 64] (the stale row pos[b] included): K = 2 * a real key row (the new key among
    them), V = +-30000"""
    B, nq, nkv, lmax, pos = case
    j = torch.arange(lmax)
    for b in range(B):
        n = pos[b] + 1
        real = torch.cat([kc[b, : n - 1], x[b, None, nq:nq + nkv]], dim=0)  # keys 0 .. pos[b]
        kc[b, n - 1:] = 2 * real[j[n - 1:] % n]
    behind = (j[None, :] >= torch.tensor(pos)[:, None])[:, :, None, None]
    vc = torch.where(behind, 30000.0 * _signs((B, lmax, nkv, 64), g), vc)
    return (x.view(B, -1).to(dt).to(dev), kc.reshape(B, lmax, nkv * 64).to(dt).contiguous().to(dev),
            vc.reshape(B, lmax, nkv * 64).to(dt).contiguous().to(dev))


def _realistic(case, ci, dt, dev):
    B, nq, nkv, lmax, pos = case
    g = torch.Generator().manual_seed(4000 + ci)
    sigma = (0.5, 1.0, 2.0)[ci % 3]
    x = torch.randn(B, nq + 2 * nkv, 64, generator=g)
    x[:, : nq + nkv] *= sigma
    kc = torch.randn(B, lmax, nkv, 64, generator=g) * sigma
    vc = torch.randn(B, lmax, nkv, 64, generator=g)
    return _with_decoys(x, kc, vc, case, g, dt, dev)


# ---------------------------------------------------------------------------------------------------------------------------
# tests

@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_case_id(c) for c in CASES])
def test_planted(gpu, ci, dt):
    """out == V[target] bit for bit, in every layout"""
    case = CASES[ci]
    B, nq, nkv, lmax, pos = case
    dev = gpu["device"]
    what = f"planted {_inst(case, dt)}: {_case_id(case)}"
    qkv, kc, vc, tgt, want = _planted(case, ci, dt, dev)
    out = _run_checked(qkv, kc, vc, case, what)
    bad = _bits(out) != _bits(want)
    if bool(bad.any()):
        b, col = _first_bad(bad)
        h = col // 64
        raise AssertionError(f"{what}: {int(bad.view(B, nq, 64).any(-1).sum())} rows are not V[target]; first: sample {b} head {h} target "
                             f"{int(tgt[b, h])} pos {pos[b]}: got key (j // 32, j % 32) = {out[b, h * 64:h * 64 + 2].tolist()}, "
                             f"dim {col % 64}: {out[b, col].item()} != {want[b, col].item()}")
    # the float64 reference agrees with the construction
    ref, _, _ = _ref(qkv, kc, vc, case)
    assert torch.equal(ref.float().to(dt), want), "the planted construction is not exact in float64"


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_case_id(c) for c in CASES])
def test_realistic(gpu, ci, dt):
    case = CASES[ci]
    dev = gpu["device"]
    key = _inst(case, dt)
    what = f"real {key}: {_case_id(case)}"
    qkv, kc, vc = _realistic(case, ci, dt, dev)
    out = _run_checked(qkv, kc, vc, case, what)
    ref, pav, sav = _ref(qkv, kc, vc, case)
    _check_single_key_rows(out, qkv, case, what)
    _check_bound(out, ref, pav, sav, dt, what, key)
    _check_global(out, ref, dt, what, key)


def _adversary(kind, case, dt, dev):
    B, nq, nkv, lmax, pos = case
    g = torch.Generator().manual_seed(lmax + len(kind))
    x = torch.randn(B, nq + 2 * nkv, 64, generator=g)
    kc = torch.randn(B, lmax, nkv, 64, generator=g)
    vc = torch.randn(B, lmax, nkv, 64, generator=g)
    u = torch.randn(64, generator=g)
    u = u / u.norm() * 8  # q . k = 64 ramp, scaled score 8 ramp
    j = torch.arange(lmax).float()
    posf = torch.tensor(pos).float()
    if kind in ("increasing", "decreasing"):
        # scores move by 40 nats over a sample's keys: the maximum sits in the last / first wave, and the far end's probabilities
        # fall below fp16's smallest subnormal
        n = (posf + 1)[:, None]
        ramp = (j[None, :] if kind == "increasing" else (n - 1 - j[None, :])) * (40.0 / (8 * n))  # [B, lmax]
        x[:, :nq] = u + 0.05 * x[:, :nq]
        kc = ramp[:, :, None, None] * u + 0.05 * kc
        x[:, nq:nq + nkv] = (ramp[torch.arange(B), torch.tensor(pos)])[:, None, None] * u + 0.05 * x[:, nq:nq + nkv]
    elif kind == "spike":
        # q = the new key (every head): it scores 0.125 |k|^2 ~ 18 +- 3, the others N(0, 2.25^2)
        kc *= 1.5
        x[:, nq:nq + nkv] *= 1.5
        x[:, :nq] = x[:, nq:nq + nkv].repeat_interleave(nq // nkv, dim=1)
    elif kind == "zero_q":
        x[:, :nq] = 0.0
    elif kind == "equal_large":
        # every key is the same row: equal scores of 0.125 * 8 * 60 = 60 (+- the storage rounding of u), P = 1 / n
        x[:, :nq] = u
        kc = (7.5 * u).expand(B, lmax, nkv, 64).clone()
        x[:, nq:nq + nkv] = 7.5 * u
    return _with_decoys(x, kc, vc, case, g, dt, dev)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ADVERSARY_CASES, ids=_case_id)
def test_adversaries(gpu, case, dt):
    """score patterns that stress the split softmax, under the per-element bound of the realistic regime"""
    B, nq, nkv, lmax, pos = case
    dev = gpu["device"]
    for kind in ("increasing", "decreasing", "spike", "zero_q", "equal_large"):
        key = _inst(case, dt) + " adversary"
        what = f"{kind} {_inst(case, dt)}: {_case_id(case)}"
        qkv, kc, vc = _adversary(kind, case, dt, dev)
        out = _run_checked(qkv, kc, vc, case, what)
        ref, pav, sav = _ref(qkv, kc, vc, case)
        k, v, pos_t = _logical_kv(qkv, kc, vc, case)
        b0 = max(range(B), key=lambda b: pos[b])  # the sample with the most keys; its head 0
        n0 = pos[b0] + 1
        s = SCALE * (k[b0, 0, :n0].double() @ qkv[b0, :64].double())
        if kind == "increasing":  # maximum among the last 64 keys; the first key 2^-24 below it: P under fp16's smallest subnormal
            assert int(s.argmax()) >= n0 - 64 and (s.max() - s[0]).item() > 17.0
        if kind == "decreasing":
            assert int(s.argmax()) < 64 and (s.max() - s[n0 - 1]).item() > 17.0
        if kind == "spike":
            assert int(s.argmax()) == n0 - 1
        if kind == "equal_large":
            assert s.min().item() > 50.0 and (s.max() - s.min()).item() < 1e-9
        if kind in ("zero_q", "equal_large"):  # uniform P: the mean of the attended V rows
            mean = v[b0, 0, :n0].double().mean(0)
            assert bool(((ref[b0, :64] - mean).abs() < 1e-9).all())
        _check_bound(out, ref, pav, sav, dt, what, key)
        _check_global(out, ref, dt, what, key, enforce=False)


def test_refusals(gpu):
    """bad arguments: TCAVT_ERR_ARG, a message starting `attn_decode:`, nothing launched (out and the caches untouched)"""
    dev = gpu["device"]
    capi = _lib()

    def call(B=2, nq=4, nkv=1, lmax=64, layout=0, dt_code=None, null=None, alloc=None):
        aB, aL = alloc or (max(B, 1), max(min(lmax, 4096), 1))
        qkv = torch.randn(aB, (nq + 2 * nkv) * 64, device=dev).to(F16)
        kc = torch.full((aB * aL, nkv * 64), float("nan"), dtype=F16, device=dev)
        vc = kc.clone()
        ob = torch.full((max(aB, 32), nq * 64), float("nan"), dtype=F16, device=dev)
        pos = torch.zeros(aB, dtype=torch.int32, device=dev)
        ptrs = dict(qkv=qkv.data_ptr(), k=kc.data_ptr(), v=vc.data_ptr(), pos=pos.data_ptr(), out=ob.data_ptr())
        if null:
            ptrs[null] = None
        rc = capi.lib().tcavt_attn_decode(ptrs["qkv"], ptrs["k"], ptrs["v"], ptrs["pos"], ptrs["out"], B, nq, nkv, lmax, SCALE,
                                          capi.F16 if dt_code is None else dt_code, layout, capi.stream_ptr())
        torch.cuda.synchronize()
        return rc, bool(torch.isnan(ob).all()) and bool(torch.isnan(kc).all()) and bool(torch.isnan(vc).all())

    rc, clean = call()
    assert rc == 0 and not clean  # the harness itself: a good call is accepted and writes
    for layout, kw in ((1, dict(B=32, nq=4)), (2, dict(B=8, nq=2)), (0, dict(B=33, nq=3, nkv=3))):
        rc, clean = call(layout=layout, **kw)
        assert rc == 0 and not clean, (layout, kw, _last_error())
    for nm in ("qkv", "k", "v", "pos", "out"):
        capi.lib().tcavt_attn_decode(64, 64, 64, 64, 64, 1, 5, 2, 64, SCALE, capi.F16, 0, capi.stream_ptr())  # (a different message)
        rc, clean = call(null=nm)
        assert rc == 1 and clean and _last_error().startswith("attn_decode:") and "null pointer" in _last_error(), (nm, _last_error())
    # the score buffer: kv_lmax + 66 * 16 floats in 64 KiB
    assert (15328 + 16 * 66) * 4 == 64 * 1024
    for name, kw in (("f32", dict(dt_code=capi.F32)), ("dtype 7", dict(dt_code=7)), ("nq % nkv", dict(nq=5, nkv=2)),
                     ("group 9", dict(nq=9, nkv=1)), ("kv_lmax 0", dict(lmax=0)), ("kv_lmax -1", dict(lmax=-1)),
                     ("kv_lmax too long", dict(lmax=15329, alloc=(2, 64))), ("layout 3", dict(layout=3)), ("layout -1", dict(layout=-1)),
                     ("layout 1, B 33", dict(layout=1, B=33)), ("layout 1, nq * 64 % 256", dict(layout=1, nq=6, nkv=2)),
                     ("layout 2, B 9", dict(layout=2, B=9))):
        capi.lib().tcavt_attn_decode(None, None, None, None, None, 1, 1, 1, 1, SCALE, capi.F16, 0, capi.stream_ptr())
        assert "null pointer" in _last_error()
        rc, clean = call(**kw)
        assert rc == 1, f"{name}: accepted (code {rc})"
        assert _last_error().startswith("attn_decode:") and "null pointer" not in _last_error(), f"{name}: tcavt_last_error = {_last_error()!r}"
        assert clean, f"{name}: a refused call wrote"


def test_report_worst_ratio(gpu):
    """(runs last in file order) prints the worst ratios measured in this session, per instantiation"""
    for k in sorted(_WORST_C):
        print(f"attn_decode  {k:24s} worst c {_WORST_C[k]:7.3f}   worst r {_WORST_R.get(k, 0.0):6.3f}")
