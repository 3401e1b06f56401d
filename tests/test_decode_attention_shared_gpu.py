"""The shared-prefix decode attention against float64 on every path: tcavt_attn_decode_shared (attn_decode_shared_kernel<fp16 |
bf16>), and tcavt_state_fanout byte for byte.

Every case calls the C entry point, in fp16 and bf16, and checks it against float64 torch on the GPU, computed from the same
16-bit inputs by the reference of tests/test_decode_attention_gpu.py (_ref) on the UNSHARED image of the inputs: row r's cache
[prefix rows 0 .. prefix_len[b] - 1 | own suffix rows 0 .. t - 1 | the new key at pos[r] = prefix_len[b] + t].  The helpers
(_bits, _ulp, _check_bound, _check_global, _guarded, the un-permutations) and the bars (_C_P = 1.0 per element, _R_GLOBAL
globally) are imported from there, not copied.  The derivation of the per-element bound there covers a probability rounded to
fp16 relative to a running maximum (it is the prefill kernels' bound, tests/test_attention_fwd_gpu.py); what this kernel adds --
the rescale of the waves' partials to one maximum, and the log-sum-exp merge of the prefix partial with the suffix -- are fp32
multiplications by exp2(m - M) <= 1, a few 2^-24 relative each, far inside the 0.05 the derivation leaves for the fp32 terms.

All six buffers live inside NaN-filled buffers with guard rows.  After every call: suffix row t of every kv head holds the qkv
row's k | v bits; every other byte of both suffix caches, the whole prefix, every guard, qkv, pos and prefix_len keep their bits;
for layouts 1 / 2 the token slots >= R are unchanged and the un-permuted rows are bit-equal to layout 0; a second launch repeats
the first bit for bit.

_paths() mirrors the host rule and the kernel's split: one workgroup of W = 8 waves per (prompt, kv head, block of 32 of the n *
group queries); wave w takes the 32-key prefix tiles w, w + 8, ...; in the suffix pass wave w takes the block's continuations
w, w + 8, ... with the group's heads that lie in the block, in chunks of H = 4, over rounds of 64 suffix keys; one instantiation
per type.  test_paths_coverage asserts from it that the case list reaches both instantiations, a padded, an exact and a second
partial query block, a wave with no key tile, waves with several tiles, group 1 / 3 / 4 / 8, a continuation whose heads straddle
two blocks, two head chunks, a wave with two continuations, a suffix of more than one round, n = 1 and all three layouts.  Cases (B, n, nq, nkv, prefix_lmax, prefix_len,
suffix_lmax); the suffix slots t are ragged per row and include 0 (only the new token) and suffix_lmax - 1:

| case | what it reaches |
|---|---|
| (3, 3, 4, 1, 48, [48, 1, 33], 5) | 12 queries: padded block; prefix_len 1 and across a 32-key tile edge |
| (2, 8, 8, 2, 100, [100, 37], 8) | exactly 32 queries |
| (1, 5, 8, 1, 70, [65], 4) | group 8, 40 queries: a full and a partial block |
| (2, 2, 4, 4, 64, [64, 63], 3) | group 1 |
| (2, 1, 8, 2, 40, [31, 32], 3) | n = 1; R = 2: layouts 0, 1, 2 |
| (1, 8, 8, 2, 2032, [2032], 16) | longest prefix, every wave several tiles |
| (4, 8, 32, 8, 272, ragged, 8) | product head counts, R = 32, layout 1 |
| (11, 3, 4, 2, 40, ragged, 4) | R = 33: layout 0 only |
| (1, 12, 6, 2, 40, [33], 70) | group 3: a continuation's heads straddle two query blocks; 12 continuations on 8 waves; suffix slots up to 69: a second round of 64 suffix keys |

Regimes: planted (bit-exact: out == V[target]; targets differ per (continuation, head) -- prefix key 0, a tile's first and last
key, prefix_len - 1, an own suffix row, the new key; decoys K = 16 * a target's code, V = +-30000 in prefix rows >= prefix_len[b],
in own suffix rows >= t and so in the stale rows of the other continuations of the prompt, whose valid rows hold other keys),
realistic (q, k ~ N(0, sigma^2), v ~ N(0, 1); the per-element and the global bound) and adversaries (maximum in the last / first
prefix tile, maximum in the suffix, a spike on the new key, q = 0, equal large scores) under the per-element bound.  The cross-check
runs the same inputs, laid out as an unshared cache, through tcavt_attn_decode under the same bound.

Measured worst ratios are written next to the bars and in profiles/attention_decode_shared_bounds.txt; test_report_worst_ratio
prints this session's (pytest -s).
"""
import pytest
import torch

import test_decode_attention_gpu as dec
from test_decode_attention_gpu import (BF16, F16, SCALE, _GUARD, _bits, _check_bound, _check_global, _dt_code, _first_bad, _guarded,
                                       _last_error, _lib, _name, _signs, from_frag, from_frag8)

pytestmark = pytest.mark.gpu

# The bars are dec._C_P (1.0) and dec._R_GLOBAL (fp16 2.0, bf16 1.25), applied by dec._check_bound / dec._check_global.
# Measured on an MI355X, worst c over the cases / over the adversaries: fp16 0.513 / 0.319, bf16 0.419 / 0.362; worst r fp16 1.375
# (adversaries, recorded only: 1.343), bf16 1.007; the same inputs through tcavt_attn_decode: c 0.757 (fp16), 0.732 (bf16).
# profiles/attention_decode_shared_bounds.txt has every case
W_WAVES = 8      # DS_W
H_CHUNK = 4      # DS_H
MAX_SUFFIX = 1152  # TCAVT_ATTN_DECODE_SHARED_MAX_SUFFIX


def _slots(R, slmax):
    """ragged suffix slots: 0 (only the new token), suffix_lmax - 1, then a stride"""
    base = [0, slmax - 1, 1, slmax // 2]
    return [min(base[r], slmax - 1) if r < len(base) else (r * 3 + 1) % slmax for r in range(R)]


def _ragged_len(B, plmax):
    base = [plmax, 1, 33, plmax - 1, 32, 31, 65]
    return [min(base[b], plmax) if b < len(base) else (b * 37 + 11) % plmax + 1 for b in range(B)]


CASES = [  # (B, n, nq, nkv, prefix_lmax, prefix_len, suffix_lmax)
    (3, 3, 4, 1, 48, [48, 1, 33], 5),
    (2, 8, 8, 2, 100, [100, 37], 8),
    (1, 5, 8, 1, 70, [65], 4),
    (2, 2, 4, 4, 64, [64, 63], 3),
    (2, 1, 8, 2, 40, [31, 32], 3),
    (1, 8, 8, 2, 2032, [2032], 16),
    (4, 8, 32, 8, 272, _ragged_len(4, 272), 8),
    (11, 3, 4, 2, 40, _ragged_len(11, 40), 4),
    (1, 12, 6, 2, 40, [33], 70),
]
ADVERSARY_CASES = [(2, 5, 8, 1, 300, [300, 257], 8)]


def _case_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}x{c[3]}x{c[4]}"


def _layouts(case):
    R, nq = case[0] * case[1], case[2]
    return [0] + ([1] if R <= 32 and (nq * 64) % 256 == 0 else []) + ([2] if R <= 8 else [])


def _paths(case):
    """tcavt_attn_decode_shared's launch and the kernel's split: query blocks per (prompt, kv head) with their real queries, and per
    prompt the number of 32-key tiles each of the W waves takes"""
    B, n, nq, nkv, plmax, plen, slmax = case
    nQ = n * (nq // nkv)
    nblk = (nQ + 31) // 32
    blocks = [min(32, nQ - 32 * i) for i in range(nblk)]
    tiles = [(min(max(p, 0), plmax) + 31) // 32 for p in plen]
    grp = nq // nkv
    suffix = []  # per block: per wave the (continuation, first head, heads) units of its suffix pass
    for i in range(nblk):
        lo, hi = 32 * i, min(32 * i + 32, nQ)
        waves = [[] for _ in range(W_WAVES)]
        for j in range(lo // grp, (hi - 1) // grp + 1):
            waves[(j - lo // grp) % W_WAVES].append((j, max(lo - j * grp, 0), min(hi - j * grp, grp) - max(lo - j * grp, 0)))
        suffix.append(waves)
    return dict(grid=B * nkv * nblk, blocks=blocks, suffix=suffix, per=[dict(tiles=t, waves=[len(range(w, t, W_WAVES)) for w in range(W_WAVES)])
                                                           for t in tiles])


def test_paths_coverage():
    layouts, groups, ns = set(), set(), set()
    padded = exact = second = empty = several = False
    for case in CASES + ADVERSARY_CASES:
        B, n, nq, nkv, plmax, plen, slmax = case
        assert len(plen) == B and all(1 <= p <= plmax for p in plen) and nq % nkv == 0 and 1 <= slmax <= MAX_SUFFIX
        t = _slots(B * n, slmax)
        assert 0 in t and (slmax - 1) in t and all(0 <= x < slmax for x in t)
        p = _paths(case)
        assert sum(p["blocks"]) == n * (nq // nkv)
        for s in p["per"]:
            assert sum(s["waves"]) == s["tiles"]  # the split covers every tile once
        units = [u for blk in p["suffix"] for wv in blk for u in wv]
        assert sorted((j, g0 + h) for j, g0, nh in units for h in range(nh)) == [(j, g) for j in range(n) for g in range(nq // nkv)]
        assert sum(1 for j, g0, nh in units if g0 == 0) == n  # every continuation's first head, so its append, exactly once
    for case in CASES:
        B, n, nq, nkv, plmax, plen, slmax = case
        p = _paths(case)
        layouts.update(_layouts(case))
        groups.add(nq // nkv)
        ns.add(n)
        padded |= p["blocks"] == [b for b in p["blocks"] if b < 32] and len(p["blocks"]) == 1
        exact |= p["blocks"] == [32]
        second |= len(p["blocks"]) == 2 and p["blocks"][0] == 32 and p["blocks"][1] < 32
        for s in p["per"]:
            empty |= 0 in s["waves"]
            several |= min(s["waves"]) >= 2
    assert padded and exact and second and empty and several
    assert layouts == {0, 1, 2} and {1, 3, 4, 8} <= groups and 1 in ns
    units = [(c, wv) for c in CASES for blk in _paths(c)["suffix"] for wv in blk]
    assert any(0 < nh < c[2] // c[3] for c, wv in units for _, _, nh in wv)  # a continuation's heads straddle two blocks
    assert any(nh > H_CHUNK for c, wv in units for _, _, nh in wv)           # two head chunks
    assert any(len(wv) >= 2 for c, wv in units) and any(len(wv) == 0 for c, wv in units)  # a wave with two continuations; with none
    assert any(max(_slots(c[0] * c[1], c[6])) >= 64 for c in CASES)          # a suffix of more than one 64-key round
    assert any(_layouts(c) == [0] for c in CASES) and any(c[0] * c[1] == 32 and 1 in _layouts(c) for c in CASES)
    lens = {p for c in CASES for p in c[5]}
    assert {1, 31, 32, 33, 2032} <= lens, sorted(lens)  # one key; a tile edge from both sides; the longest


# ---------------------------------------------------------------------------------------------------------------------------
# launching with poisoned buffers; the unshared image and the float64 reference

def _launch(x, case, t, layout, what):
    """One tcavt_attn_decode_shared call on fresh copies of all buffers; asserts every invariant that does not need the reference.
    x = (qkv, pk, pv, sk, sv).  Returns out [R, nq * 64] (un-permuted for layouts 1 and 2)."""
    capi = _lib()
    B, n, nq, nkv, plmax, plen, slmax = case
    qkv, pk0, pv0, sk0, sv0 = x
    R, dt, dev, W, w = B * n, qkv.dtype, qkv.device, nq * 64, nkv * 64
    what = f"{what} layout {layout}"
    plen_t = torch.tensor(plen, dtype=torch.int32, device=dev)
    pos_t = plen_t.repeat_interleave(n) + torch.tensor(t, dtype=torch.int32, device=dev)
    pkb, pkv = _guarded(pk0.view(B * plmax, w))
    pvb, pvv = _guarded(pv0.view(B * plmax, w))
    skb, skv = _guarded(sk0.view(R * slmax, w))
    svb, svv = _guarded(sv0.view(R * slmax, w))
    qbuf, q = _guarded(qkv)
    rows = R if layout == 0 else 8 if layout == 2 else 16 * ((R + 15) // 16)
    obuf = torch.full((rows + 2 * _GUARD, W), float("nan"), dtype=dt, device=dev)
    out = obuf[_GUARD:_GUARD + rows]
    before = [b.clone() for b in (pkb, pvb, skb, svb, qbuf, obuf, pos_t, plen_t)]
    rc = capi.lib().tcavt_attn_decode_shared(q.data_ptr(), pkv.data_ptr(), pvv.data_ptr(), plen_t.data_ptr(), skv.data_ptr(), svv.data_ptr(),
                                             pos_t.data_ptr(), out.data_ptr(), B, n, nq, nkv, plmax, slmax, SCALE, _dt_code(dt), layout,
                                             capi.stream_ptr())
    torch.cuda.synchronize()
    capi.check(rc, what)
    pk1, pv1, sk1, sv1, q1, o1, pos1, plen1 = before
    assert torch.equal(_bits(qbuf), _bits(q1)) and torch.equal(pos_t, pos1) and torch.equal(plen_t, plen1), f"{what}: qkv / pos / prefix_len modified"
    assert torch.equal(_bits(pkb), _bits(pk1)) and torch.equal(_bits(pvb), _bits(pv1)), f"{what}: the prefix was written"
    for nm, buf, b0 in (("out", obuf, o1), ("suffix_k", skb, sk1), ("suffix_v", svb, sv1)):
        assert torch.equal(_bits(buf[:_GUARD]), _bits(b0[:_GUARD])) and torch.equal(_bits(buf[-_GUARD:]), _bits(b0[-_GUARD:])), \
            f"{what}: write into the guard rows of {nm}"
    at = torch.zeros(R, slmax, dtype=torch.bool, device=dev)
    at[torch.arange(R, device=dev), torch.tensor(t, device=dev)] = True
    at = at.view(R * slmax)
    for nm, c, c0, col in (("suffix_k", skv, sk1[_GUARD:-_GUARD], nq * 64), ("suffix_v", svv, sv1[_GUARD:-_GUARD], (nq + nkv) * 64)):
        same = (_bits(c) == _bits(c0)).all(-1)
        assert bool(same[~at].all()), f"{what}: {nm} row {_first_bad((~same & ~at).view(R, slmax))} (row, slot) was written"
        assert torch.equal(_bits(c[at]), _bits(qkv[:, col:col + w])), f"{what}: {nm} row t is not the qkv row's bits"
    if layout == 0:
        res = out
    else:
        full = from_frag(out.reshape(-1), rows, W) if layout == 1 else from_frag8(out.reshape(-1), W)
        assert torch.equal(_bits(full[R:]), _bits(torch.full_like(full[R:], float("nan")))), f"{what}: token slots >= R written"
        res = full[:R].contiguous()
    assert torch.isfinite(res).all(), f"{what}: {int((~torch.isfinite(res)).sum())} non-finite (unwritten) out elements"
    return res.clone()


def _run_checked(x, case, t, what):
    """layout 0 twice, then every other legal layout: bit-equal results.  Returns out [R, nq * 64]."""
    a = _launch(x, case, t, 0, what)
    b = _launch(x, case, t, 0, what + " (second launch)")
    assert torch.equal(_bits(a), _bits(b)), f"{what}: two launches differ"
    for layout in _layouts(case)[1:]:
        o = _launch(x, case, t, layout, what)
        bad = _bits(o) != _bits(a)
        assert not bool(bad.any()), f"{what}: layout {layout} differs from layout 0 at (row, column) {_first_bad(bad)}"
    return a


def _unshared(x, case, t):
    """The same inputs as tcavt_attn_decode sees them: (k_cache, v_cache [R, lmax, nkv * 64], its case (R, nq, nkv, lmax, pos)) with
    row r = [prefix rows < prefix_len[b] | own suffix rows < t]; the rows from pos[r] on hold K = 0, V = 30000 (never attended)."""
    B, n, nq, nkv, plmax, plen, slmax = case
    qkv, pk, pv, sk, sv = x
    R, w, lmax = B * n, nkv * 64, plmax + slmax
    kc = torch.zeros(R, lmax, w, dtype=qkv.dtype, device=qkv.device)
    vc = torch.full((R, lmax, w), 30000.0, dtype=qkv.dtype, device=qkv.device)
    for r in range(R):
        b, p = r // n, plen[r // n]
        kc[r, :p], vc[r, :p] = pk[b, :p], pv[b, :p]
        kc[r, p:p + t[r]], vc[r, p:p + t[r]] = sk[r, :t[r]], sv[r, :t[r]]
    return kc, vc, (R, nq, nkv, lmax, [plen[r // n] + t[r] for r in range(R)])


def _reference(x, case, t):
    kc, vc, ucase = _unshared(x, case, t)
    return dec._ref(x[0], kc, vc, ucase)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs

def _planted(case, ci, dt, dev):
    """(qkv, pk, pv, sk, sv) in dt on dev, the slots t and want [R, nq * 64]"""
    B, n, nq, nkv, plmax, plen, slmax = case
    R, grp = B * n, nq // nkv
    t = _slots(R, slmax)
    g = torch.Generator().manual_seed(5000 + ci)
    rb = torch.arange(R) // n
    cp, cs, cn = _signs((B, nkv, plmax, 64), g), _signs((R, nkv, slmax, 64), g), _signs((R, nkv, 64), g)
    val = lambda shape: torch.randint(-64, 65, shape, generator=g).float() / 16
    vp, vs, vn = val((B, nkv, plmax, 64)), val((R, nkv, slmax, 64)), val((R, nkv, 64))
    jp, js = torch.arange(plmax), torch.arange(slmax)
    vp[..., 0], vp[..., 1] = (jp // 32).float(), (jp % 32).float()   # which prefix key
    vs[..., 0], vs[..., 1] = 100.0, js.float()                       # which suffix key
    vn[..., 0], vn[..., 1] = 200.0, torch.arange(R).float()[:, None]  # the new key of which row
    kvh = torch.arange(nq) // grp
    qcode, want = torch.zeros(R, nq, 64), torch.zeros(R, nq, 64)
    kinds = []
    for r in range(R):
        p = plen[r // n]
        last_tile = (p - 1) // 32 * 32
        pats = [("p", 0), ("p", last_tile), ("p", min(31, p - 1)), ("p", p - 1), ("s", max(t[r] - 1, 0)), ("n", 0), ("s", 0),
                ("p", min(32, p - 1))]
        for hq in range(nq):
            kind, j = pats[(hq + r + ci) % len(pats)]
            if kind == "s" and t[r] == 0:
                kind = "n"
            kinds.append(kind)
            h = int(kvh[hq])
            if kind == "p":
                qcode[r, hq], want[r, hq] = cp[r // n, h, j], vp[r // n, h, j]
            elif kind == "s":
                qcode[r, hq], want[r, hq] = cs[r, h, j], vs[r, h, j]
            else:
                qcode[r, hq], want[r, hq] = cn[r, h], vn[r, h]
    assert {"p", "s", "n"} <= set(kinds)
    # every attended key but the target scores 8 * dot <= 320, 192 below the target's 512 (the target itself: dot 64)
    tp = torch.tensor(plen)[rb]
    tt = torch.tensor(t)
    dp = torch.einsum("rhd,rhjd->rhj", qcode, cp[rb][:, kvh])
    ds = torch.einsum("rhd,rhjd->rhj", qcode, cs[:, kvh])
    dn = torch.einsum("rhd,rhd->rh", qcode, cn[:, kvh])
    dp = dp.masked_fill(jp[None, None, :] >= tp[:, None, None], -99.0)
    ds = ds.masked_fill(js[None, None, :] >= tt[:, None, None], -99.0)
    alld = torch.cat([dp, ds, dn[..., None]], -1)
    assert bool(((alld == 64).sum(-1) == 1).all()) and alld[alld != 64].max().item() <= 40, "planted codes too close"
    # decoys: 16 * the code of a target of the (prompt, kv head)'s queries, in turn; +-30000 in V
    qall = qcode.view(B, n, nkv, grp, 64).permute(0, 2, 1, 3, 4).reshape(B, nkv, n * grp, 64)  # [B, nkv, query, 64]
    dec_p = qall[:, :, jp % (n * grp)]  # [B, nkv, plmax, 64]
    dec_s = qall[rb][:, :, (js + 1) % (n * grp)]  # [R, nkv, slmax, 64]
    pad_p = (jp[None, :] >= torch.tensor(plen)[:, None])[:, None, :, None]
    pad_s = (js[None, :] >= tt[:, None])[:, None, :, None]
    kp = torch.where(pad_p, 16 * dec_p, 8 * cp)
    ks = torch.where(pad_s, 16 * dec_s, 8 * cs)
    vpd = torch.where(pad_p, 30000.0 * _signs(vp.shape, g), vp)
    vsd = torch.where(pad_s, 30000.0 * _signs(vs.shape, g), vs)
    qkv = torch.cat([8 * qcode, 8 * cn, vn], dim=1).view(R, -1)
    lay = lambda a: a.permute(0, 2, 1, 3).reshape(a.shape[0], a.shape[2], nkv * 64).to(dt).contiguous().to(dev)
    assert torch.equal(qkv.to(dt).float(), qkv) and torch.equal(want.to(dt).float(), want)  # exact in dt
    return (qkv.to(dt).to(dev), lay(kp), lay(vpd), lay(ks), lay(vsd)), t, want.view(R, nq * 64).to(dt).to(dev)


def _finish(q, kn, vn, kp, vp, ks, vs, case, t, g, dt, dev):
    """logical tensors (q [R, nq, 64], kn / vn [R, nkv, 64], kp / vp [B, plmax, nkv, 64], ks / vs [R, slmax, nkv, 64]) -> the five
    buffers, with decoys (K = 2 * a real key row of the owner, V = +-30000) in prefix rows >= prefix_len[b] and suffix rows >= t"""
    B, n, nq, nkv, plmax, plen, slmax = case
    R = B * n
    kp, vp, ks, vs = kp.clone(), vp.clone(), ks.clone(), vs.clone()
    for b in range(B):
        p = plen[b]
        kp[b, p:] = 2 * kp[b, torch.arange(plmax - p) % p]
        vp[b, p:] = 30000.0 * _signs((plmax - p, nkv, 64), g)
    for r in range(R):
        real = torch.cat([ks[r, :t[r]], kn[r][None]], 0)
        ks[r, t[r]:] = 2 * real[torch.arange(slmax - t[r]) % (t[r] + 1)]
        vs[r, t[r]:] = 30000.0 * _signs((slmax - t[r], nkv, 64), g)
    qkv = torch.cat([q, kn, vn], dim=1).reshape(R, -1)
    f = lambda a: a.reshape(a.shape[0], a.shape[1], nkv * 64).to(dt).contiguous().to(dev)
    return qkv.to(dt).to(dev), f(kp), f(vp), f(ks), f(vs)


def _realistic(case, ci, dt, dev):
    B, n, nq, nkv, plmax, plen, slmax = case
    R = B * n
    g = torch.Generator().manual_seed(6000 + ci)
    sigma = (0.5, 1.0, 2.0)[ci % 3]
    rn = lambda *s: torch.randn(*s, generator=g)
    return _finish(rn(R, nq, 64) * sigma, rn(R, nkv, 64) * sigma, rn(R, nkv, 64), rn(B, plmax, nkv, 64) * sigma, rn(B, plmax, nkv, 64),
                   rn(R, slmax, nkv, 64) * sigma, rn(R, slmax, nkv, 64), case, _slots(R, slmax), g, dt, dev), _slots(R, slmax)


def _adversary(kind, case, dt, dev):
    B, n, nq, nkv, plmax, plen, slmax = case
    R = B * n
    t = _slots(R, slmax)
    g = torch.Generator().manual_seed(plmax + len(kind))
    rn = lambda *s: torch.randn(*s, generator=g)
    q, kn, vn, kp, vp, ks, vs = (rn(R, nq, 64), rn(R, nkv, 64), rn(R, nkv, 64), rn(B, plmax, nkv, 64), rn(B, plmax, nkv, 64),
                                 rn(R, slmax, nkv, 64), rn(R, slmax, nkv, 64))
    u = rn(64)
    u = u / u.norm() * 8  # q . k = 64 * ramp, scaled score 8 * ramp
    lens = torch.tensor(plen).float()[:, None]
    jp = torch.arange(plmax).float()[None, :]
    if kind in ("last_tile", "first_tile", "suffix_max"):
        # scores move by 40 nats over the prefix (maximum in its last / first tile; the far end's probabilities fall under fp16's
        # smallest subnormal); the suffix and the new key sit low -- or, suffix_max, 10 nats above the whole prefix
        ramp = (jp if kind != "first_tile" else (lens - 1 - jp)) * (5.0 / lens)  # [B, plmax], 0 .. 5
        q = u + 0.05 * q
        kp = ramp[:, :, None, None] * u + 0.05 * kp
        top = 6.25 if kind == "suffix_max" else 1.0
        ks = top * u + 0.05 * ks
        kn = top * u + 0.05 * kn
    elif kind == "spike":
        kp, ks, kn = 1.5 * kp, 1.5 * ks, 1.5 * kn
        q = kn.repeat_interleave(nq // nkv, dim=1)
    elif kind == "zero_q":
        q = torch.zeros_like(q)
    elif kind == "equal_large":
        q = u.expand(R, nq, 64).clone()
        kp, ks, kn = (7.5 * u).expand_as(kp).clone(), (7.5 * u).expand_as(ks).clone(), (7.5 * u).expand_as(kn).clone()
    return _finish(q, kn, vn, kp, vp, ks, vs, case, t, g, dt, dev), t


# ---------------------------------------------------------------------------------------------------------------------------
# tests

@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_case_id(c) for c in CASES])
def test_planted(gpu, ci, dt):
    """out == V[target] bit for bit, in every layout"""
    case = CASES[ci]
    B, n, nq = case[:3]
    what = f"planted {_name(dt)}: {_case_id(case)}"
    x, t, want = _planted(case, ci, dt, gpu["device"])
    out = _run_checked(x, case, t, what)
    bad = _bits(out) != _bits(want)
    if bool(bad.any()):
        r, col = _first_bad(bad)
        raise AssertionError(f"{what}: {int(bad.view(B * n, nq, 64).any(-1).sum())} (row, head) pairs are not V[target]; first: row {r} "
                             f"(prompt {r // n}, prefix_len {case[5][r // n]}, slot {t[r]}) head {col // 64}: got tags "
                             f"{out[r, col // 64 * 64:col // 64 * 64 + 2].tolist()} want {want[r, col // 64 * 64:col // 64 * 64 + 2].tolist()}")
    ref, _, _ = _reference(x, case, t)
    assert torch.equal(ref.float().to(dt), want), "the planted construction is not exact in float64"


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_case_id(c) for c in CASES])
def test_realistic(gpu, ci, dt):
    case = CASES[ci]
    key = f"shared {_name(dt)}"
    what = f"real {key}: {_case_id(case)}"
    x, t = _realistic(case, ci, dt, gpu["device"])
    out = _run_checked(x, case, t, what)
    ref, pav, sav = _reference(x, case, t)
    _check_bound(out, ref, pav, sav, dt, what, key)
    _check_global(out, ref, dt, what, key)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ADVERSARY_CASES, ids=_case_id)
def test_adversaries(gpu, case, dt):
    """score patterns that stress the online softmax, the waves' merge and the prefix / suffix merge, under the per-element bound"""
    B, n, nq, nkv, plmax, plen, slmax = case
    for kind in ("last_tile", "first_tile", "suffix_max", "spike", "zero_q", "equal_large"):
        key = f"shared {_name(dt)} adversary"
        what = f"{kind} {_name(dt)}: {_case_id(case)}"
        x, t = _adversary(kind, case, dt, gpu["device"])
        out = _run_checked(x, case, t, what)
        ref, pav, sav = _reference(x, case, t)
        kc, vc, ucase = _unshared(x, case, t)
        r0 = 1  # slot suffix_lmax - 1: the longest suffix; its head 0
        n0 = ucase[4][r0] + 1
        k = torch.cat([kc[r0, :n0 - 1, :64], x[0][r0, nq * 64:nq * 64 + 64][None]], 0).double()
        s = SCALE * (k @ x[0][r0, :64].double())
        p0 = plen[0]
        if kind == "last_tile":
            assert p0 - 32 <= int(s.argmax()) < p0 and (s.max() - s[0]).item() > 17.0
        if kind == "first_tile":
            assert int(s.argmax()) < 32 and (s.max() - s[p0 - 1]).item() > 17.0
        if kind == "suffix_max":
            assert int(s.argmax()) >= p0 and (s.max() - s[:p0].max()).item() > 5.0
        if kind == "spike":
            assert int(s.argmax()) == n0 - 1
        if kind == "equal_large":
            assert s.min().item() > 50.0 and (s.max() - s.min()).item() < 1e-9
        _check_bound(out, ref, pav, sav, dt, what, key)
        _check_global(out, ref, dt, what, key, enforce=False)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("ci", [0, 2, 6], ids=[_case_id(CASES[i]) for i in (0, 2, 6)])
def test_cross_check_unshared(gpu, ci, dt):
    """the same inputs as an unshared cache through tcavt_attn_decode: the same reference, the same bound (no bit equality)"""
    case = CASES[ci]
    x, t = _realistic(case, ci, dt, gpu["device"])
    ref, pav, sav = _reference(x, case, t)
    kc, vc, ucase = _unshared(x, case, t)
    pos_t = torch.tensor(ucase[4], dtype=torch.int32, device=gpu["device"])
    got = dec._launch(x[0], kc, vc, pos_t, ucase, 0, f"unshared {_case_id(case)}")
    _check_bound(got, ref, pav, sav, dt, f"cross-check unshared {_name(dt)}: {_case_id(case)}", f"unshared {_name(dt)} cross-check")
    out = _launch(x, case, t, 0, f"cross-check shared {_case_id(case)}")
    _check_bound(out, ref, pav, sav, dt, f"cross-check shared {_name(dt)}: {_case_id(case)}", f"shared {_name(dt)}")


def test_refusals(gpu):
    """bad arguments: TCAVT_ERR_ARG, a message starting `attn_decode_shared:`, nothing launched (every buffer untouched)"""
    dev = gpu["device"]
    capi = _lib()

    def call(B=2, n=2, nq=4, nkv=1, plmax=40, slmax=4, layout=0, dt_code=None, null=None, off=None, alloc=None):
        aB, an, aP, aS = alloc or (max(B, 1), max(n, 1), max(plmax, 1), max(slmax, 1))
        aR = aB * an
        qkv = torch.randn(aR, (nq + 2 * nkv) * 64, device=dev).to(F16)
        nanbuf = lambda rows, cols: torch.full((rows, cols), float("nan"), dtype=F16, device=dev)
        pk, pv, sk, sv = nanbuf(aB * aP, nkv * 64), nanbuf(aB * aP, nkv * 64), nanbuf(aR * aS, nkv * 64), nanbuf(aR * aS, nkv * 64)
        pk[:] = 1.0
        pv[:] = 1.0
        ob = nanbuf(max(aR, 32) + 1, nq * 64)
        pos = torch.full((aR,), 3, dtype=torch.int32, device=dev)
        plen = torch.full((aB,), 3, dtype=torch.int32, device=dev)
        ptrs = dict(qkv=qkv.data_ptr(), pk=pk.data_ptr(), pv=pv.data_ptr(), plen=plen.data_ptr(), sk=sk.data_ptr(), sv=sv.data_ptr(),
                    pos=pos.data_ptr(), out=ob.data_ptr())
        if null:
            ptrs[null] = None
        if off:
            ptrs[off] += 8  # 8-byte aligned only
        rc = capi.lib().tcavt_attn_decode_shared(ptrs["qkv"], ptrs["pk"], ptrs["pv"], ptrs["plen"], ptrs["sk"], ptrs["sv"], ptrs["pos"],
                                                 ptrs["out"], B, n, nq, nkv, plmax, slmax, SCALE, capi.F16 if dt_code is None else dt_code,
                                                 layout, capi.stream_ptr())
        torch.cuda.synchronize()
        clean = bool(torch.isnan(ob).all()) and bool(torch.isnan(sk).all()) and bool(torch.isnan(sv).all()) and bool((pk == 1).all()) and bool((pv == 1).all())
        return rc, clean

    rc, clean = call()
    assert rc == 0 and not clean  # the harness itself: a good call is accepted and writes
    for layout, kw in ((1, dict(B=4, n=8, nq=4)), (2, dict(B=2, n=4, nq=2)), (0, dict(B=11, n=3, nq=3, nkv=3))):
        rc, clean = call(layout=layout, **kw)
        assert rc == 0 and not clean, (layout, kw, _last_error())
    for nm in ("qkv", "pk", "pv", "plen", "sk", "sv", "pos", "out"):
        capi.lib().tcavt_attn_decode_shared(64, 64, 64, 64, 64, 64, 64, 64, 1, 1, 5, 2, 8, 8, SCALE, capi.F16, 0, capi.stream_ptr())
        rc, clean = call(null=nm)
        assert rc == 1 and clean and _last_error().startswith("attn_decode_shared:") and "null pointer" in _last_error(), (nm, _last_error())
    for name, kw in (("f32", dict(dt_code=capi.F32)), ("nq % nkv", dict(nq=5, nkv=2)), ("group 9", dict(nq=9, nkv=1)), ("B 0", dict(B=0)),
                     ("n 0", dict(n=0)), ("n -1", dict(n=-1)), ("prefix_lmax 0", dict(plmax=0)), ("suffix_lmax 0", dict(slmax=0)),
                     ("suffix_lmax too long", dict(slmax=MAX_SUFFIX + 1, alloc=(2, 2, 40, 4))), ("layout 3", dict(layout=3)),
                     ("layout -1", dict(layout=-1)), ("layout 1, R 33", dict(layout=1, B=11, n=3)),
                     ("layout 1, nq * 64 % 256", dict(layout=1, nq=6, nkv=2)), ("layout 2, R 9", dict(layout=2, B=3, n=3)),
                     ("unaligned qkv", dict(off="qkv")), ("unaligned prefix_k", dict(off="pk")), ("unaligned prefix_v", dict(off="pv")),
                     ("unaligned suffix_k", dict(off="sk")), ("unaligned suffix_v", dict(off="sv")), ("unaligned out", dict(off="out"))):
        capi.lib().tcavt_attn_decode_shared(None, None, None, None, None, None, None, None, 1, 1, 1, 1, 1, 1, SCALE, capi.F16, 0, capi.stream_ptr())
        assert "null pointer" in _last_error()
        rc, clean = call(**kw)
        assert rc == 1, f"{name}: accepted (code {rc})"
        assert _last_error().startswith("attn_decode_shared:") and "null pointer" not in _last_error(), f"{name}: tcavt_last_error = {_last_error()!r}"
        assert clean, f"{name}: a refused call wrote"
    rc, clean = call(slmax=MAX_SUFFIX, alloc=(2, 2, 40, MAX_SUFFIX))  # the longest suffix the entry accepts
    assert rc == 0 and not clean, _last_error()


@pytest.mark.parametrize("V", [48, 50], ids=["V48", "V50"])
@pytest.mark.parametrize("n", [1, 3], ids=["n1", "n3"])
def test_state_fanout_is_a_byte_copy_and_writes_nothing_else(gpu, n, V):
    """tcavt_state_fanout: the state and first logits of tcavt_kv_fanout, and not one byte besides (sentinels everywhere)"""
    from tcavt_amd import ops

    dev = gpu["device"]
    B, n_ids, cap, n_image = 3, 5, 9, 16
    R = B * n
    g = torch.Generator().manual_seed(n * 100 + V)
    ids = torch.randint(0, 1000, (B, n_ids), generator=g).to(dev)
    kv_len = torch.tensor([16 + 5, 16 + 2, 16 + 4], dtype=torch.int32, device=dev)
    src = torch.randn(B, V, generator=g).to(dev)
    src.view(torch.int32)[0, 1] = 0x7FC01234  # a NaN payload travels bit for bit
    G = 2
    lbuf = torch.full(((R + 2 * G) * V + 8,), -7.0, device=dev)
    off = (-(lbuf.data_ptr() // 4 + G * V)) % 4  # the first destination row 16-byte aligned, whatever V is
    logits = lbuf[off + G * V: off + (G + R) * V].view(R, V)
    assert logits.data_ptr() % 16 == 0
    hbuf = torch.full((R + 2 * G, cap), -5, dtype=torch.int64, device=dev)
    sbuf = {k: torch.full((R + 2 * G,), -3, dtype=torch.int32, device=dev) for k in ("hist_len", "pos", "finished")}
    hist = hbuf[G:G + R]
    st = {k: v[G:G + R] for k, v in sbuf.items()}
    before = (ids.clone(), kv_len.clone(), src.clone())
    ops.state_fanout(n, ids, kv_len, n_image, src, logits, hist, st["hist_len"], st["pos"], st["finished"])
    torch.cuda.synchronize()
    assert torch.equal(ids, before[0]) and torch.equal(kv_len, before[1]) and torch.equal(_bits(src), _bits(before[2]))
    rb = torch.arange(R, device=dev) // n
    assert torch.equal(_bits(logits), _bits(src[rb])), "logits rows are not the source's bits"
    want_l = torch.full_like(lbuf, -7.0)
    want_l[off + G * V: off + (G + R) * V] = src[rb].reshape(-1)
    assert torch.equal(_bits(lbuf), _bits(want_l)), "a logits element outside the R rows was written"
    want_h = torch.full_like(hbuf, -5)
    want_h[G:G + R, :n_ids] = ids[rb]
    assert torch.equal(hbuf, want_h), "history: prompt ids in the first n_ids columns of the R rows, nothing else"
    for k, want in (("hist_len", kv_len[rb] - n_image), ("pos", kv_len[rb]), ("finished", torch.zeros(R, dtype=torch.int32, device=dev))):
        full = torch.full_like(sbuf[k], -3)
        full[G:G + R] = want
        assert torch.equal(sbuf[k], full), k


def test_report_worst_ratio(gpu):
    """(runs last in file order) prints the worst ratios measured in this session, per instantiation"""
    for k in sorted(dec._WORST_C):
        print(f"attn_decode_shared  {k:32s} worst c {dec._WORST_C[k]:7.3f}   worst r {dec._WORST_R.get(k, 0.0):6.3f}")
