"""tcavt_attn_decode_multi: T consecutive positions of each of S sequences on one cache per sequence, against the existing kernel.

Shapes of test_decode_step_gpu.py's model: 8 / 2 heads of 64, kv_lmax = 200.  Cases (S, T) in {(1, 2), (1, 8), (2, 4), (3, 5),
(4, 8), (8, 4), (8, 1)}, every sequence's base = pos_rows[s * T] from {0, 63, 64, 130, 200 - T} (every case sees all five), fp16 and
bf16, all three out_layouts where legal (1: S * T <= 32, 2: S * T <= 8).  Inputs: qkv and the cache rows below base random; every
row from base on is a decoy (K = 4 * a real row of the sequence, V = +-30000) -- the T rows the launch overwrites as well as the
rows at and behind base + T -- so a read of a cache row at or beyond base changes the output; NaN guard rows around out and both
caches.

The reference is the existing kernel: T sequential tcavt_attn_decode launches at B = S on a copy of the caches, launch j with the
qkv rows s * T + j and pos = base + j.  Asserted, bit for bit: out row s * T + j equals launch j's row s; both caches equal the
reference's caches after its T launches (so rows base .. base + T - 1 hold the qkv rows' k | v, checked against qkv directly too,
and every other row keeps its bits); guards, qkv and pos_rows are unchanged; slots >= S * T of a fragment-major out are unchanged;
layouts 1 and 2 un-permuted equal layout 0.  T = 1 is compared with the one plain launch it must be.
One shape beyond the model's (32 / 8 heads, S = 3, T = 6: 576 workgroups) reaches the instantiation without the value-row prefetch,
which the plain launches at B = 3 do not use: the prefetch moves loads, not arithmetic, so the bits are equal there too.

One case, (3, 5) in fp16 and bf16, is also held to float64 at the per-element bound of test_decode_attention_gpu.py (its _ref and
_check_bound, c = 1.0): the float64 attention of the one query per row over the cached rows below base and the new keys 0 .. j."""
import pytest
import torch

import test_decode_attention_gpu as A

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
KV_LMAX, SCALE, GUARD = 200, 0.125, 3
CASES = [(1, 2), (1, 8), (2, 4), (3, 5), (4, 8), (8, 4), (8, 1)]


def _bases(S, T, rnd):
    all_b = [0, 63, 64, 130, KV_LMAX - T]
    return [all_b[(s + rnd * S) % 5] for s in range(S)]


def _rounds(S):
    return -(-5 // S)


def _inputs(S, T, nq, nkv, bases, dt, dev, seed):
    w, nqkv = nkv * 64, (nq + 2 * nkv) * 64
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(S * T, nqkv, generator=g)
    kc, vc = torch.randn(S, KV_LMAX, w, generator=g), torch.randn(S, KV_LMAX, w, generator=g)
    base = torch.tensor(bases)
    j = torch.arange(KV_LMAX)
    behind = (j[None, :] >= base[:, None])[:, :, None]
    src = j[None, :] % base.clamp_min(1)[:, None]
    kc = torch.where(behind, 4 * torch.gather(kc, 1, src[:, :, None].expand_as(kc)), kc)
    sign = (torch.randint(0, 2, vc.shape, generator=g) * 2 - 1).float()
    vc = torch.where(behind, 30000.0 * sign, vc)
    pos_rows = (base[:, None] + torch.arange(T)[None, :]).reshape(-1).to(torch.int32)
    return qkv.to(dt).to(dev), kc.to(dt).to(dev), vc.to(dt).to(dev), pos_rows.to(dev)


def _guarded(x):
    buf = torch.full((x.shape[0] + 2 * GUARD, x.shape[1]), float("nan"), dtype=x.dtype, device=x.device)
    buf[GUARD:GUARD + x.shape[0]] = x
    return buf, buf[GUARD:GUARD + x.shape[0]]


def _multi(qkv, kc0, vc0, pos_rows, S, T, nq, nkv, layout, what):
    """one launch on fresh guarded copies -> (out [R, nq * 64] un-permuted, k cache, v cache)"""
    from tcavt_amd import ops

    R, W, w = S * T, nq * 64, nkv * 64
    dt, dev = qkv.dtype, qkv.device
    kbuf, kc = _guarded(kc0.reshape(S * KV_LMAX, w))
    vbuf, vc = _guarded(vc0.reshape(S * KV_LMAX, w))
    qbuf, q = _guarded(qkv)
    rows = R if layout == 0 else 8 if layout == 2 else 16 * ((R + 15) // 16)
    obuf = torch.full((rows + 2 * GUARD, W), float("nan"), dtype=dt, device=dev)
    out = obuf[GUARD:GUARD + rows]
    k0, v0, q0, o0, p0 = kbuf.clone(), vbuf.clone(), qbuf.clone(), obuf.clone(), pos_rows.clone()
    ops.attn_decode_multi(q, kc, vc, pos_rows, out, S, T, nq, nkv, KV_LMAX, SCALE, out_layout=layout)
    torch.cuda.synchronize()
    assert torch.equal(A._bits(qbuf), A._bits(q0)) and torch.equal(pos_rows, p0), f"{what}: qkv / pos_rows modified"
    for nm, buf, b0 in (("out", obuf, o0), ("k_cache", kbuf, k0), ("v_cache", vbuf, v0)):
        assert torch.equal(A._bits(buf[:GUARD]), A._bits(b0[:GUARD])) and torch.equal(A._bits(buf[-GUARD:]), A._bits(b0[-GUARD:])), \
            f"{what}: write into the guard rows of {nm}"
    if layout == 0:
        res = out
    else:
        full = A.from_frag(out.reshape(-1), rows, W) if layout == 1 else A.from_frag8(out.reshape(-1), W)
        assert torch.equal(A._bits(full[R:]), A._bits(torch.full_like(full[R:], float("nan")))), f"{what}: token slots >= S * T written"
        res = full[:R].contiguous()
    assert torch.isfinite(res).all(), f"{what}: non-finite (unwritten) out elements"
    return res.clone(), kc.clone().view(S, KV_LMAX, w), vc.clone().view(S, KV_LMAX, w)


def _sequential(qkv, kc0, vc0, bases, S, T, nq, nkv):
    """the reference: T plain launches at B = S on one copy of the caches -> (out [R, nq * 64], k cache, v cache)"""
    from tcavt_amd import ops

    dev = qkv.device
    kc, vc = kc0.clone(), vc0.clone()
    out = torch.zeros(S * T, nq * 64, dtype=qkv.dtype, device=dev)
    base = torch.tensor(bases, dtype=torch.int32, device=dev)
    for j in range(T):
        q_j = qkv.view(S, T, -1)[:, j].contiguous()
        o_j = torch.zeros(S, nq * 64, dtype=qkv.dtype, device=dev)
        ops.attn_decode(q_j, kc, vc, (base + j).contiguous(), o_j, S, nq, nkv, KV_LMAX, SCALE)
        out.view(S, T, -1)[:, j] = o_j
    torch.cuda.synchronize()
    return out, kc, vc


def _check_case(dev, S, T, nq, nkv, dt, layouts, rounds):
    w = nkv * 64
    for rnd in rounds:
        bases = _bases(S, T, rnd)
        qkv, kc0, vc0, pos_rows = _inputs(S, T, nq, nkv, bases, dt, dev, 1000 * S + 10 * T + rnd)
        want, kc_ref, vc_ref = _sequential(qkv, kc0, vc0, bases, S, T, nq, nkv)
        for layout in layouts:
            what = f"S={S} T={T} nq={nq} {A._name(dt)} bases={bases} layout {layout}"
            got, kc, vc = _multi(qkv, kc0, vc0, pos_rows, S, T, nq, nkv, layout, what)
            bad = A._bits(got) != A._bits(want)
            assert not bool(bad.any()), f"{what}: out differs from the sequential launches at (row, column) {A._first_bad(bad)}"
            assert torch.equal(A._bits(kc), A._bits(kc_ref)) and torch.equal(A._bits(vc), A._bits(vc_ref)), f"{what}: caches differ"
            for s, b in enumerate(bases):  # rows base .. base + T - 1 are the qkv rows' k | v; every other row keeps its bits
                rows = qkv[s * T:(s + 1) * T]
                assert torch.equal(A._bits(kc[s, b:b + T]), A._bits(rows[:, nq * 64:nq * 64 + w])), f"{what}: k rows of sequence {s}"
                assert torch.equal(A._bits(vc[s, b:b + T]), A._bits(rows[:, nq * 64 + w:])), f"{what}: v rows of sequence {s}"
                keep = torch.ones(KV_LMAX, dtype=torch.bool, device=dev)
                keep[b:b + T] = False
                assert torch.equal(A._bits(kc[s][keep]), A._bits(kc0[s][keep])) and torch.equal(A._bits(vc[s][keep]), A._bits(vc0[s][keep])), \
                    f"{what}: a cache row outside base .. base + T - 1 of sequence {s} was written"


def _layouts(R):
    return [0] + ([1] if R <= 32 else []) + ([2] if R <= 8 else [])


def test_case_list():
    for S, T in CASES:
        seen = {b for rnd in range(_rounds(S)) for b in _bases(S, T, rnd)}
        assert seen == {0, 63, 64, 130, KV_LMAX - T} and all(b + T - 1 <= KV_LMAX - 1 for b in seen), (S, T)
    assert [_layouts(S * T) for S, T in CASES] == [[0, 1, 2], [0, 1, 2], [0, 1, 2], [0, 1], [0, 1], [0, 1], [0, 1, 2]]


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("S,T", CASES)
def test_bit_equal_to_sequential_plain_launches(gpu, S, T, dt):
    _check_case(gpu["device"], S, T, 8, 2, dt, _layouts(S * T), range(_rounds(S)))


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_without_value_prefetch(gpu, dt):
    """S * T * nq = 576 > 512: the multi launch runs without the value-row prefetch, the plain launches at B = 3 with it"""
    _check_case(gpu["device"], 3, 6, 32, 8, dt, [0, 1], [0, 1])


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_against_float64(gpu, dt):
    """(3, 5) against the float64 attention of every row over its sequence's keys, at test_decode_attention_gpu.py's bound"""
    dev = gpu["device"]
    S, T, nq, nkv = 3, 5, 8, 2
    bases = [63, 64, 130]
    qkv, kc0, vc0, pos_rows = _inputs(S, T, nq, nkv, bases, dt, dev, 77)
    got, _, _ = _multi(qkv, kc0, vc0, pos_rows, S, T, nq, nkv, 0, f"float64 {A._name(dt)}")
    # every row's own view of the keys: its sequence's cache with rows base .. base + j - 1 taken from the qkv rows before it
    R, w = S * T, nkv * 64
    kc, vc = kc0.repeat_interleave(T, dim=0).clone(), vc0.repeat_interleave(T, dim=0).clone()
    for s, b in enumerate(bases):
        for j in range(T):
            kc[s * T + j, b:b + j] = qkv[s * T:s * T + j, nq * 64:nq * 64 + w]
            vc[s * T + j, b:b + j] = qkv[s * T:s * T + j, nq * 64 + w:]
    case = (R, nq, nkv, KV_LMAX, pos_rows.tolist())
    ref, pav, sav = A._ref(qkv, kc, vc, case)
    key = f"multi {A._name(dt)}"
    try:
        A._check_bound(got, ref, pav, sav, dt, f"attn_decode_multi (3, 5) {A._name(dt)}", key)
    finally:
        A._WORST_C.pop(key, None)  # (that file's report lists its own instantiations)
