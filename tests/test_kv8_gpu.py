"""The two kernels of the FP8 KV cache ("KV8") through their C entry points, in fp16 and bf16: tcavt_kv_store8 (the prefill store)
and tcavt_attn_decode8 (the decode attention on the FP8 planes).  The format is quant.kv8_quantize: per cached 64-element row of a
kv head 64 e4m3fn codes + 2 E8M0 scale bytes, planes head-major [B][nkv][kv_lmax][64 | 2].

Every buffer sits inside guards (0xA5 bytes around the uint8 planes, NaN rows around qkv and out).  After every attention call:
guards intact; every plane byte outside row pos[b] unchanged; row pos[b] == quantize_mx of the qkv row's k | v; qkv and pos
unchanged; token slots >= B of out unchanged in layouts 1 and 2; layouts bit-equal to layout 0; a second launch repeats the first;
a sample with pos[b] == 0 returns the new v bit for bit.

_paths8() mirrors the NEW kernel's launch rule: KS = min(16, ceil(kv_lmax / 64)) waves per (sample, query head) split the m = pos[b]
CACHED keys in chunks of ceil(ceil(m / KS) / 64) * 64 (64 up to m = 1024, 128 beyond); the new key is wave 0's, from qkv.  One
instantiation per 16-bit type (no prefetch variant).  test_paths_coverage asserts from that mirror alone what the case list reaches.

Regimes:
- planted (bit-exact): the planes are built from codes and scale bytes directly.  Keys are +-1 codes (0x38 / 0xB8) with scale byte
  130, i.e. +-8, the query 8 * the target's signs: the target scores 512, every other key 8 * dot <= 320 (dot <= 40 asserted), so
  every other probability is exactly 0 and out == the target's dequantised V row bit for bit.  V: random finite e4m3 codes (without
  0x80: 0 + 1 * -0 is +0 in any accumulation), scale bytes in [120, 134] -- every value exact in fp16 and bf16.  Rows at and behind pos[b]: K = 16 * a target's signs (scale byte 131),
  V = +-448 * 2^7 (the largest codes, scale byte 134).  The new key / value in qkv are exactly representable in the format.
- realistic / adversaries: the inputs of test_decode_attention_gpu.py pushed through kv8_quantize; reference = float64 attention on
  kv8_dequantize(..., float64) with row pos[b] from qkv; the same per-element bound
      |got - ref| <= c * 2^-11 (P|V|)_d + 2^-25 sum_j |V_jd| + ulp_out(ref),  c = 1.0,
  and the same global bar r = 2.0 (fp16) / 1.25 (bf16).  The derivation (test_decode_attention_gpu.py) rests on the arithmetic
  contract alone -- exact dequantisation, fp32 scores and sums, one global (max, sum), probabilities rounded to fp16 once, fp32
  accumulation -- which tcavt_attn_decode8 keeps.  Measured worst c / r: profiles/attention_decode_kv8_bounds.txt.
"""
import pytest
import torch

import test_decode_attention_gpu as T

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
SCALE = 0.125
_GB = 256  # guard bytes around a plane (keeps the planes 16-byte aligned)
_C1, _CM1 = 0x38, 0xB8  # e4m3fn codes of +1 and -1
_WORST_C, _WORST_R = {}, {}


def _quant():
    from tcavt_amd import quant

    return quant


# ---------------------------------------------------------------------------------------------------------------------------
# the store

STORE_SHAPES = [(3, 24, 40, 4, 1), (2, 70, 72, 8, 2), (1, 130, 136, 32, 8)]  # (B, L, kv_lmax, nq, nkv)


def _guarded_bytes(n, dev):
    buf = torch.full((n + 2 * _GB,), 0xA5, dtype=torch.uint8, device=dev)
    return buf, buf[_GB:_GB + n]


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", STORE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_store(gpu, shape, dt):
    capi, quant = T._lib(), _quant()
    B, L, lmax, nq, nkv = shape
    dev = gpu["device"]
    g = torch.Generator().manual_seed(B * 1000 + L)
    ld, w = (nq + 2 * nkv) * 64, nkv * 64
    x = torch.randn(B * L, ld, generator=g) * torch.logspace(-2, 2, B * L)[:, None]
    x[1, nq * 64 + 5] = float("inf")  # a row with an inf (k, head 0, block 0)
    x[2, nq * 64 + w + 32:nq * 64 + w + 64] = 0.0  # an all-zero block (v, head 0, block 1)
    x[3, nq * 64:nq * 64 + 32] = torch.randn(32, generator=g) * 2.0 ** -20  # magnitudes near 2^-20: fp16 subnormals
    x = x.to(dt)
    qbuf, q = T._guarded(x.to(dev))
    planes = [_guarded_bytes(B * nkv * lmax * per, dev) for per in (64, 2, 64, 2)]
    q0, p0 = qbuf.clone(), [b.clone() for b, _ in planes]
    rc = capi.lib().tcavt_kv_store8(q.data_ptr(), B, L, lmax, nq, nkv, T._dt_code(dt), *[v.data_ptr() for _, v in planes], capi.stream_ptr())
    torch.cuda.synchronize()
    capi.check(rc, "kv_store8")
    assert torch.equal(T._bits(qbuf), T._bits(q0)), "qkv modified"
    xk = x[:, nq * 64:nq * 64 + w].reshape(B, L, w)
    xv = x[:, nq * 64 + w:].reshape(B, L, w)
    want = quant.kv8_quantize(xk) + quant.kv8_quantize(xv)  # (k codes, k scales, v codes, v scales), each [B, nkv, L, per]
    if dt == F16:
        assert int(want[1][0, 0, 3 % L, 0]) - 127 < -20  # the subnormal block carries its own small scale
    assert bool((want[0][0, 0, 1, :32] == 0x7F).all())
    for (buf, view), b0, wnt, nm, per in zip(planes, p0, want, ("k_codes", "k_scales", "v_codes", "v_scales"), (64, 2, 64, 2)):
        assert torch.equal(buf[:_GB], b0[:_GB]) and torch.equal(buf[-_GB:], b0[-_GB:]), f"{nm}: write into the guards"
        got = view.view(B, nkv, lmax, per).cpu()
        assert torch.equal(got[:, :, :L], wnt), f"{nm}: not kv8_quantize ({int((got[:, :, :L] != wnt).sum())} bytes differ)"
        assert bool((got[:, :, L:] == 0xA5).all()), f"{nm}: positions >= L written"


# ---------------------------------------------------------------------------------------------------------------------------
# the attention: host-rule mirror and the case list

def _paths8(B, nq, kv_lmax, pos):
    """tcavt_attn_decode8's launch and attn_decode8_kernel's split of the CACHED keys: KS, LDS bytes, and per sample n = pos + 1, the
    cached count m, chunk and the number of cached keys each of the KS waves holds (wave 0 also holds the new key)"""
    KS = min(16, (kv_lmax + 63) // 64)
    lds = (kv_lmax + KS * 66) * 4
    per = []
    for p in pos:
        m = min(max(p, 0), kv_lmax - 1)
        chunk = ((m + KS - 1) // KS + 63) // 64 * 64
        per.append(dict(n=m + 1, m=m, chunk=chunk, keys=[max(0, min(chunk, m - k * chunk)) for k in range(KS)]))
    return dict(KS=KS, lds=lds, per=per)


CASES = [  # (B, nq, nkv, kv_lmax, pos)
    (3, 4, 1, 48, [0, 20, 47]),
    (4, 4, 4, 104, [63, 64, 65, 103]),
    (4, 8, 1, 136, [0, 64, 128, 135]),
    (4, 4, 1, 1088, [1024, 1087, 1025, 127]),
    (3, 8, 2, 2048, [2047, 1500, 0]),
    (17, 32, 8, 104, T._ragged(17, 104)),
    (33, 16, 2, 72, T._ragged(33, 72)),
]
ADVERSARY_CASES = [(2, 8, 1, 2048, [2047, 1029]), (17, 32, 8, 200, T._ragged(17, 200))]
_layouts, _case_id = T._layouts, T._case_id


def test_paths_coverage():
    """from the mirror of the new kernel's rule alone: both instantiations (every case runs in fp16 and bf16), every split count the rule
    yields at these lengths, both chunk sizes and both sides of the length where the chunk changes (m = 1024 | 1025), a wave with no key
    and one with exactly one key, n in {1, 64, 65}, groups 1, 4, 8, all three layouts"""
    ks, chunks, layouts, groups, ms = set(), set(), set(), set(), set()
    empty = one = full = False
    for case in CASES + ADVERSARY_CASES:
        B, nq, nkv, lmax, pos = case
        assert len(pos) == B and all(0 <= p <= lmax - 1 for p in pos) and nq % nkv == 0 and nq // nkv <= 8
        p = _paths8(B, nq, lmax, pos)
        assert p["lds"] <= 64 * 1024 and 1 <= p["KS"] <= 16
        for s in p["per"]:
            assert sum(s["keys"]) == s["m"], (case, s)  # the split covers every cached key once
    for case in CASES:
        B, nq, nkv, lmax, pos = case
        p = _paths8(B, nq, lmax, pos)
        ks.add(p["KS"])
        groups.add(nq // nkv)
        layouts.update(_layouts(case))
        for s in p["per"]:
            ms.add(s["m"])
            if s["m"]:
                chunks.add(s["chunk"])
            empty |= 0 in s["keys"][1:] and s["m"] > 0
            one |= 1 in s["keys"][1:]
            full |= p["KS"] == 16 and s["m"] > 0 and all(k == s["chunk"] for k in s["keys"])
    assert ks == {min(16, (c[3] + 63) // 64) for c in CASES} == {1, 2, 3, 16}, ks
    assert chunks == {64, 128}, chunks
    assert {1024, 1025} <= ms  # both sides of the chunk change: the last m with one round per wave, the first with two
    assert empty and one and full
    assert {0, 63, 64} <= ms  # n = 1, 64, 65
    assert any(s["m"] == 64 and s["keys"][1] == 0 for c in CASES for s in _paths8(c[0], c[1], c[3], c[4])["per"])  # exactly one full round
    assert layouts == {0, 1, 2}
    assert {1, 4, 8} <= groups, groups
    assert any(16 < c[0] <= 32 and 1 in _layouts(c) for c in CASES) and any(c[0] > 32 for c in CASES)
    assert any(_layouts(c) == [0, 1, 2] for c in CASES)
    assert any(s["m"] == 2047 for c in ADVERSARY_CASES for s in _paths8(c[0], c[1], c[3], c[4])["per"])


# ---------------------------------------------------------------------------------------------------------------------------
# launching with guarded buffers

def _launch(qkv, planes0, pos_t, case, layout, what):
    """One tcavt_attn_decode8 call on fresh copies of the planes (kc, ks, vc, vs: uint8 [B, nkv, lmax, 64 | 2]); asserts every invariant that
    needs no reference.  Returns out [B, nq * 64] (un-permuted for layouts 1 and 2)."""
    capi, quant = T._lib(), _quant()
    B, nq, nkv, lmax, pos = case
    dt, dev, W, w = qkv.dtype, qkv.device, nq * 64, nkv * 64
    what = f"{what} layout {layout}"
    bufs = []
    for p0 in planes0:
        buf, view = _guarded_bytes(p0.numel(), dev)
        view.copy_(p0.reshape(-1))
        bufs.append((buf, view))
    qbuf, q = T._guarded(qkv)
    rows = B if layout == 0 else 8 if layout == 2 else 16 * ((B + 15) // 16)
    obuf = torch.full((rows + 2 * T._GUARD, W), float("nan"), dtype=dt, device=dev)
    out = obuf[T._GUARD:T._GUARD + rows]
    b0, q0, o0, p0_ = [b.clone() for b, _ in bufs], qbuf.clone(), obuf.clone(), pos_t.clone()
    rc = capi.lib().tcavt_attn_decode8(q.data_ptr(), *[v.data_ptr() for _, v in bufs], pos_t.data_ptr(), out.data_ptr(), B, nq, nkv, lmax,
                                       SCALE, T._dt_code(dt), layout, capi.stream_ptr())
    torch.cuda.synchronize()
    capi.check(rc, what)
    assert torch.equal(T._bits(qbuf), T._bits(q0)) and torch.equal(pos_t, p0_), f"{what}: qkv / pos modified"
    assert torch.equal(T._bits(obuf[:T._GUARD]), T._bits(o0[:T._GUARD])) and torch.equal(T._bits(obuf[-T._GUARD:]), T._bits(o0[-T._GUARD:])), \
        f"{what}: write into the guard rows of out"
    # the planes: row pos[b] of every kv head is quantize_mx of the qkv row's k | v, every other byte keeps its value
    at = torch.zeros(B, nkv, lmax, dtype=torch.bool, device=dev)
    at[torch.arange(B, device=dev), :, pos_t.long()] = True
    qc = qkv.cpu()  # (the format's definition runs on the host)
    newk = [t.to(dev) for t in quant.kv8_quantize(qc[:, None, nq * 64:nq * 64 + w]) + quant.kv8_quantize(qc[:, None, nq * 64 + w:])]  # [B, nkv, 1, per]
    for (buf, view), old, nw, nm, per in zip(bufs, b0, newk, ("k_codes", "k_scales", "v_codes", "v_scales"), (64, 2, 64, 2)):
        assert torch.equal(buf[:_GB], old[:_GB]) and torch.equal(buf[-_GB:], old[-_GB:]), f"{what}: write into the guards of {nm}"
        now, was = view.view(B, nkv, lmax, per), old[_GB:-_GB].view(B, nkv, lmax, per)
        same = (now == was).all(-1)
        assert bool(same[~at].all()), f"{what}: {nm} (sample, kv head, row) {T._first_bad(~same & ~at)} was written"
        assert torch.equal(now[at].view(B, nkv, per), nw.view(B, nkv, per)), f"{what}: {nm} row pos[b] is not quantize_mx of the qkv row"
    if layout == 0:
        res = out
    else:
        full = T.from_frag(out.reshape(-1), rows, W) if layout == 1 else T.from_frag8(out.reshape(-1), W)
        assert torch.equal(T._bits(full[B:]), T._bits(torch.full_like(full[B:], float("nan")))), f"{what}: token slots >= B written"
        res = full[:B].contiguous()
    assert torch.isfinite(res).all(), f"{what}: {int((~torch.isfinite(res)).sum())} non-finite (unwritten) out elements"
    return res.clone()


def _run_checked(qkv, planes, case, what):
    """layout 0 twice, then every other legal layout: bit-equal results.  Returns out [B, nq * 64]."""
    pos_t = torch.tensor(case[4], dtype=torch.int32, device=qkv.device)
    a = _launch(qkv, planes, pos_t, case, 0, what)
    b = _launch(qkv, planes, pos_t, case, 0, what + " (second launch)")
    assert torch.equal(T._bits(a), T._bits(b)), f"{what}: two launches differ"
    for layout in _layouts(case)[1:]:
        o = _launch(qkv, planes, pos_t, case, layout, what)
        bad = T._bits(o) != T._bits(a)
        assert not bool(bad.any()), f"{what}: layout {layout} differs from layout 0 at (sample, column) {T._first_bad(bad)}"
    return a


def _ref(qkv, planes, case):
    """float64 attention on kv8_dequantize(planes, float64) with row pos[b] taken from qkv: out, P|V|, sum |V| (T._ref)"""
    quant = _quant()
    kd = quant.kv8_dequantize(planes[0], planes[1], torch.float64)
    vd = quant.kv8_dequantize(planes[2], planes[3], torch.float64)
    return T._ref(qkv.double(), kd, vd, case)


def _check_bound(got, ref, pav, sav, dt, what, key):
    T._check_bound(got, ref, pav, sav, dt, what, key)  # (bar T._C_P = 1.0; records into T._WORST_C)
    _WORST_C[key] = max(_WORST_C.get(key, -1.0), T._WORST_C[key])


def _check_global(got, ref, dt, what, key, enforce=True):
    T._check_global(got, ref, dt, what, key, enforce)  # (bar T._R_GLOBAL: 2.0 fp16, 1.25 bf16)
    _WORST_R[key] = max(_WORST_R.get(key, 0.0), T._WORST_R.get(key, 0.0))


# ---------------------------------------------------------------------------------------------------------------------------
# inputs

def _planted(case, ci, dt, dev):
    """qkv (dt) and the four planes, built from codes and scale bytes; targets [B, nq]; want [B, nq * 64] (dt)"""
    quant = _quant()
    B, nq, nkv, lmax, pos = case
    grp = nq // nkv
    g = torch.Generator().manual_seed(3000 + ci)
    per = _paths8(B, nq, lmax, pos)["per"]
    sign = T._signs((B, nkv, lmax, 64), g)
    vcode = torch.randint(0, 256, (B, nkv, lmax, 64), generator=g).to(torch.uint8)
    vcode = torch.where((vcode & 0x7F) == 0x7F, torch.full_like(vcode, _C1), vcode)  # finite codes only
    vcode = torch.where(vcode == 0x80, torch.zeros_like(vcode), vcode)  # (no -0: a sum of products that starts at +0 cannot return it)
    vsb = torch.randint(120, 135, (B, nkv, lmax, 2), generator=g).to(torch.uint8)
    j = torch.arange(lmax)
    post = torch.tensor(pos)
    tgt = torch.zeros(B, nq, dtype=torch.long)
    for b in range(B):
        m, chunk = per[b]["m"], per[b]["chunk"]
        first = (m - 1) // chunk * chunk if m > 0 else 0  # first key of the last non-empty wave
        pats = [m, 0, min(63, m), min(64, m), first, max(first - 1, 0)]
        for hq in range(nq):
            which = (hq + b + ci) % (len(pats) + 1)
            tgt[b, hq] = pats[which] if which < len(pats) else int(torch.randint(0, m + 1, (1,), generator=g))
    assert bool((tgt <= post[:, None]).all()) and bool((tgt >= 0).all())
    kvh = torch.arange(nq) // grp
    qsign = sign[torch.arange(B)[:, None], kvh[None, :], tgt]  # [B, nq, 64]
    dots = torch.einsum("bhd,bhjd->bhj", qsign, sign[:, kvh])
    other = (j[None, None, :] <= post[:, None, None]) & (j[None, None, :] != tgt[..., None])
    assert dots[other].numel() == 0 or dots[other].max().item() <= 40, f"planted codes too close: dot {dots[other].max().item()}"
    behind = (j[None, :] >= post[:, None])[:, None, :, None]  # [B, 1, lmax, 1] (the stale row pos[b] included)
    turn = torch.arange(nkv)[:, None] * grp + j[None, :] % grp
    decoy = qsign[torch.arange(B)[:, None, None], turn[None]]  # [B, nkv, lmax, 64]
    ksign = torch.where(behind, decoy, sign)
    kc = torch.where(ksign > 0, torch.full_like(vcode, _C1), torch.full_like(vcode, _CM1))
    ks = torch.where(behind.expand(B, nkv, lmax, 2), torch.tensor(131, dtype=torch.uint8), torch.tensor(130, dtype=torch.uint8))
    big = torch.where(T._signs((B, nkv, lmax, 64), g) > 0, torch.tensor(0x7E, dtype=torch.uint8), torch.tensor(0xFE, dtype=torch.uint8))
    vc = torch.where(behind, big, vcode)
    vs = torch.where(behind.expand(B, nkv, lmax, 2), torch.tensor(134, dtype=torch.uint8), vsb)
    vtrue = quant.dequantize_mx(vcode.reshape(-1, 64), vsb.reshape(-1, 2), torch.float64).view(B, nkv, lmax, 64)  # (before the decoys)
    assert torch.equal(vtrue.to(dt).double(), vtrue)  # every dequantised value is exact in dt
    ar = torch.arange(B)
    x = torch.cat([8 * qsign.double(), 8 * sign[ar, :, post].double(), vtrue[ar, :, post]], dim=1)  # [B, nq + 2 nkv, 64]
    qkv = x.view(B, -1).to(dt)
    assert torch.equal(qkv.double(), x.view(B, -1))
    # the new key / value are exactly representable under the format
    nk = qkv[:, None, nq * 64:]
    assert torch.equal(quant.kv8_dequantize(*quant.kv8_quantize(nk), dt), nk)
    want = vtrue[ar[:, None], kvh[None, :], tgt].view(B, nq * 64).to(dt)
    return qkv.to(dev), [t.contiguous().to(dev) for t in (kc, ks, vc, vs)], tgt, want.to(dev)


def _quantised(qkv, kc16, vc16):
    """the 16-bit test's caches [B, lmax, nkv * 64] pushed through kv8_quantize"""
    quant = _quant()
    return [t.contiguous().to(qkv.device) for t in quant.kv8_quantize(kc16.cpu()) + quant.kv8_quantize(vc16.cpu())]


# ---------------------------------------------------------------------------------------------------------------------------
# tests

@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_case_id(c) for c in CASES])
def test_planted(gpu, ci, dt):
    """out == the target's dequantised V row bit for bit, in every layout, twice"""
    case = CASES[ci]
    B, nq, nkv, lmax, pos = case
    what = f"planted kv8 {T._name(dt)}: {_case_id(case)}"
    qkv, planes, tgt, want = _planted(case, ci, dt, gpu["device"])
    out = _run_checked(qkv, planes, case, what)
    bad = T._bits(out) != T._bits(want)
    if bool(bad.any()):
        b, col = T._first_bad(bad)
        h = col // 64
        raise AssertionError(f"{what}: {int(bad.view(B, nq, 64).any(-1).sum())} rows are not V[target]; first: sample {b} head {h} target "
                             f"{int(tgt[b, h])} pos {pos[b]} dim {col % 64}: {out[b, col].item()} != {want[b, col].item()}")
    ref, _, _ = _ref(qkv, planes, case)
    assert torch.equal(ref.float().to(dt), want), "the planted construction is not exact in float64"


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_case_id(c) for c in CASES])
def test_realistic(gpu, ci, dt):
    case = CASES[ci]
    key = f"kv8 {T._name(dt)}"
    what = f"real {key}: {_case_id(case)}"
    qkv, kc16, vc16 = T._realistic(case, ci, dt, gpu["device"])
    planes = _quantised(qkv, kc16, vc16)
    out = _run_checked(qkv, planes, case, what)
    ref, pav, sav = _ref(qkv, planes, case)
    T._check_single_key_rows(out, qkv, case, what)
    _check_bound(out, ref, pav, sav, dt, what, key)
    _check_global(out, ref, dt, what, key)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ADVERSARY_CASES, ids=_case_id)
def test_adversaries(gpu, case, dt):
    """increasing / decreasing / spike / zero-q / equal-large scores, quantised, under the same per-element bound"""
    for kind in ("increasing", "decreasing", "spike", "zero_q", "equal_large"):
        key = f"kv8 {T._name(dt)} adversary"
        what = f"{kind} {key}: {_case_id(case)}"
        qkv, kc16, vc16 = T._adversary(kind, case, dt, gpu["device"])
        planes = _quantised(qkv, kc16, vc16)
        out = _run_checked(qkv, planes, case, what)
        ref, pav, sav = _ref(qkv, planes, case)
        _check_bound(out, ref, pav, sav, dt, what, key)
        _check_global(out, ref, dt, what, key, enforce=False)


def test_refusals(gpu):
    """bad arguments: TCAVT_ERR_ARG, a message starting `attn_decode8:` / `kv_store8:`, nothing written"""
    dev = gpu["device"]
    capi = T._lib()

    def call(B=2, nq=4, nkv=1, lmax=64, layout=0, dt_code=None, null=None, alloc=None):
        aB, aL = alloc or (max(B, 1), max(min(lmax, 4096), 1))
        qkv = torch.randn(aB, (nq + 2 * nkv) * 64, device=dev).to(F16)
        pl = [torch.full((aB * nkv * aL * per,), 0xA5, dtype=torch.uint8, device=dev) for per in (64, 2, 64, 2)]
        ob = torch.full((max(aB, 32), nq * 64), float("nan"), dtype=F16, device=dev)
        pos = torch.zeros(aB, dtype=torch.int32, device=dev)
        ptrs = dict(qkv=qkv.data_ptr(), kc=pl[0].data_ptr(), ks=pl[1].data_ptr(), vc=pl[2].data_ptr(), vs=pl[3].data_ptr(),
                    pos=pos.data_ptr(), out=ob.data_ptr())
        if null:
            ptrs[null] = None
        rc = capi.lib().tcavt_attn_decode8(ptrs["qkv"], ptrs["kc"], ptrs["ks"], ptrs["vc"], ptrs["vs"], ptrs["pos"], ptrs["out"], B, nq, nkv,
                                           lmax, SCALE, capi.F16 if dt_code is None else dt_code, layout, capi.stream_ptr())
        torch.cuda.synchronize()
        return rc, bool(torch.isnan(ob).all()) and all(bool((p == 0xA5).all()) for p in pl)

    rc, clean = call()
    assert rc == 0 and not clean  # the harness itself: a good call is accepted and writes
    for layout, kw in ((1, dict(B=32, nq=4)), (2, dict(B=8, nq=2)), (0, dict(B=33, nq=3, nkv=3))):
        rc, clean = call(layout=layout, **kw)
        assert rc == 0 and not clean, (layout, kw, T._last_error())
    for nm in ("qkv", "kc", "ks", "vc", "vs", "pos", "out"):
        capi.lib().tcavt_attn_decode8(64, 64, 64, 64, 64, 64, 64, 1, 5, 2, 64, SCALE, capi.F16, 0, capi.stream_ptr())  # (a different message)
        rc, clean = call(null=nm)
        assert rc == 1 and clean and T._last_error().startswith("attn_decode8:") and "null pointer" in T._last_error(), (nm, T._last_error())
    assert (15328 + 16 * 66) * 4 == 64 * 1024  # the kernel's own limit: the score buffer
    for name, kw in (("f32", dict(dt_code=capi.F32)), ("dtype 7", dict(dt_code=7)), ("nq % nkv", dict(nq=5, nkv=2)),
                     ("group 9", dict(nq=9, nkv=1)), ("kv_lmax 0", dict(lmax=0)), ("kv_lmax -1", dict(lmax=-1)),
                     ("kv_lmax too long", dict(lmax=15329, alloc=(2, 64))), ("layout 3", dict(layout=3)), ("layout -1", dict(layout=-1)),
                     ("layout 1, B 33", dict(layout=1, B=33)), ("layout 1, nq * 64 % 256", dict(layout=1, nq=6, nkv=2)),
                     ("layout 2, B 9", dict(layout=2, B=9))):
        capi.lib().tcavt_attn_decode8(None, None, None, None, None, None, None, 1, 1, 1, 1, SCALE, capi.F16, 0, capi.stream_ptr())
        assert "null pointer" in T._last_error()
        rc, clean = call(**kw)
        assert rc == 1, f"{name}: accepted (code {rc})"
        assert T._last_error().startswith("attn_decode8:") and "null pointer" not in T._last_error(), f"{name}: {T._last_error()!r}"
        assert clean, f"{name}: a refused call wrote"

    def store(B=2, L=8, lmax=8, nq=4, nkv=1, dt_code=capi.F16, null=None):
        qkv = torch.randn(B * L, (nq + 2 * nkv) * 64, device=dev).to(F16)
        pl = [torch.full((B * nkv * max(lmax, L) * per,), 0xA5, dtype=torch.uint8, device=dev) for per in (64, 2, 64, 2)]
        ptrs = [qkv.data_ptr()] + [p.data_ptr() for p in pl]
        if null is not None:
            ptrs[null] = None
        rc = capi.lib().tcavt_kv_store8(ptrs[0], B, L, lmax, nq, nkv, dt_code, *ptrs[1:], capi.stream_ptr())
        torch.cuda.synchronize()
        return rc, all(bool((p == 0xA5).all()) for p in pl)

    rc, clean = store()
    assert rc == 0 and not clean
    for name, kw in (("null qkv", dict(null=0)), ("null k_scales", dict(null=2)), ("null v_codes", dict(null=3)), ("f32", dict(dt_code=capi.F32)),
                     ("kv_lmax < L", dict(lmax=7)), ("kv_lmax 0", dict(lmax=0)), ("B 0", dict(B=0)), ("nkv 0", dict(nkv=0))):
        rc, clean = store(**{k: v for k, v in kw.items() if k != "B"}) if kw.get("B") != 0 else (
            capi.lib().tcavt_kv_store8(64, 0, 8, 8, 4, 1, capi.F16, 64, 64, 64, 64, capi.stream_ptr()), True)
        assert rc == 1 and clean and T._last_error().startswith("kv_store8:"), (name, rc, T._last_error())


def test_report_worst_ratio(gpu):
    """(runs last in file order) prints the worst ratios measured in this session, per instantiation"""
    for k in sorted(_WORST_C):
        print(f"attn_decode8  {k:24s} worst c {_WORST_C[k]:7.3f}   worst r {_WORST_R.get(k, 0.0):6.3f}")
