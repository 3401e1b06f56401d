"""The streaming decoder attention (tcavt_attn_causal_gqa_stream: attn_causal_gqa_stream_kernel<fp16 | bf16>) against float64.

The reference, the two input regimes, the NaN-guarded launch buffers and the bound forms are those of
test_attention_fwd_gpu.py (imported, not copied); the bars are its bars: _C_P = 1.0, _R_GLOBAL, _LSE_ULPS = 16.  They carry
over because the arithmetic per key is the same; the only term that grows with L is the fp32 rescale of O once per key tile,
at most (L / 32) * 2^-24 relative: under 1 % of the 2^-11 term at 2048.

_paths() mirrors the host rule of tcavt_attn_causal_gqa_stream: 2 * group * 64 threads, one instantiation per type, a
workgroup per (sample, kv head, chunk of 64 queries) that walks key chunks of 256.  The query-chunk count changes between
L = 64 k and 64 k + 1, the key-chunk count between 256 k and 256 k + 1: EDGE_CASES has both sides of every such edge up to
2048 (one sample, few heads, the group cycling through 1, 3, 4, 8).  test_paths_coverage asserts from the lists alone that
they reach all of it.  Cases (B, L, nq, nkv, kv_len):

| case | group | why |
|---|---|---|
| (3, 1, 4, 1, [1, 1, 0]) | 4 | L = 1; a sample with no key |
| (3, 33, 2, 2, [33, 32, 1]) | 1 | second block of one query; kv_len on a tile edge |
| (2, 256, 8, 2, [256, 170]) | 4 | one full key chunk, four query chunks |
| (2, 257, 4, 1, [257, 256]) | 4 | second key chunk of one key; kv_len on the chunk edge and one past it |
| (2, 545, 8, 2, [545, 513]) | 4 | first length the decoder stack hands over; kv_len one past a chunk edge |
| (3, 1040, 8, 2, [1040, 700, 100]) | 4 | stage 1's length; kv_len inside chunk 0 while L spans 5 chunks |
| (2, 1040, 3, 1, [1024, 0]) | 3 | group 3; kv_len on a chunk edge; a sample with no key |
| (1, 1040, 1, 1, [1040]) | 1 | group 1 (two waves) |
| (1, 800, 6, 2, [768]) | 3 | kv_len on a chunk edge, 32 padded queries behind it |
| (2, 2048, 4, 1, [2047, 513]) | 4 | the cap; L % 32 = 0 with kv_len % 32 = 31 |
| (1, 2048, 8, 1, [2048]) | 8 | group 8 (1024 threads) at the cap |

Planted regime at these lengths: random +-1 codes of length 64 break the setup's `dot <= 40` assertion too often (5 sigma over
2 * 10^6 pairs at 2048), so the codes are drawn with rejection (_far_codes); the assertion itself stays where it is.

Further: two launches bit-equal, with and without lse bit-equal, inputs unchanged, guards intact (_run_checked); at L in
{300, 544} the stream and the resident entry both meet the float64 bound on the same inputs (bit equality not required);
refused calls write nothing; the adversaries of the forward file at (1, 1040, 4, 1).

Measured worst ratios: profiles/attention_stream_bounds.txt; test_report_worst_ratio prints this session's (pytest -s).
"""
import contextlib

import pytest
import torch

import test_attention_fwd_gpu as fwd
from test_attention_fwd_gpu import BF16, F16, F32, SCALE, _bits, _case_id, _name

gpu_test = pytest.mark.gpu
QC, KC, MAX_L = 64, 256, 2048


def _paths(L, nq, nkv):
    """tcavt_attn_causal_gqa_stream's launch: group, threads, query chunks (workgroups per sample and kv head), key chunks"""
    group = nq // nkv
    return dict(group=group, threads=2 * group * 64, nqc=-(-L // QC), nkc=-(-L // KC))


CASES = [  # (B, L, nq, nkv, kv_len)
    (3, 1, 4, 1, [1, 1, 0]),
    (3, 33, 2, 2, [33, 32, 1]),
    (2, 256, 8, 2, [256, 170]),
    (2, 257, 4, 1, [257, 256]),
    (2, 545, 8, 2, [545, 513]),
    (3, 1040, 8, 2, [1040, 700, 100]),
    (2, 1040, 3, 1, [1024, 0]),
    (1, 1040, 1, 1, [1040]),
    (1, 800, 6, 2, [768]),
    (2, 2048, 4, 1, [2047, 513]),
    (1, 2048, 8, 1, [2048]),
]
_EDGE_HEADS = [(1, 1), (3, 1), (4, 1), (8, 1)]
# both sides of every length at which the query-chunk count (64 k | 64 k + 1) or the key-chunk count (256 k | 256 k + 1) changes
EDGE_CASES = [(1, L, *_EDGE_HEADS[(k + d) % 4], [L - (k % 3)]) for k in range(1, MAX_L // QC) for d, L in enumerate((QC * k, QC * k + 1))]
ALL_CASES = CASES + EDGE_CASES
ADVERSARY_CASE = (1, 1040, 4, 1, [1040])
BOTH_ENTRIES = [(2, 300, 8, 2, [300, 257]), (2, 544, 4, 1, [544, 513])]


def test_paths_coverage():
    """from the lists alone (no GPU): required lengths, every chunk-count edge on both sides, groups, kv_len patterns"""
    Ls = {c[1] for c in ALL_CASES}
    for B, L, nq, nkv, kv in ALL_CASES + [ADVERSARY_CASE] + BOTH_ENTRIES:
        assert 1 <= B <= 3 and nq <= 16 and 1 <= L <= MAX_L and len(kv) == B and all(0 <= n <= L for n in kv) and nq % nkv == 0
        assert nq // nkv <= 8
    assert {1, 33, 256, 257, 545, 1040, 2048} <= Ls
    # every length at which the host rule changes the grid or the kernel its key-chunk walk, both sides
    for L in range(1, MAX_L):
        if _paths(L, 4, 1)["nqc"] != _paths(L + 1, 4, 1)["nqc"] or _paths(L, 4, 1)["nkc"] != _paths(L + 1, 4, 1)["nkc"]:
            assert L in Ls and L + 1 in Ls, L
    assert _paths(64, 4, 1)["nqc"] == 1 and _paths(65, 4, 1)["nqc"] == 2 and _paths(256, 4, 1)["nkc"] == 1 and _paths(257, 4, 1)["nkc"] == 2
    assert _paths(2048, 8, 1) == dict(group=8, threads=1024, nqc=32, nkc=8)
    groups = {c[2] // c[3] for c in CASES}
    assert {1, 3, 4, 8} <= groups and {c[2] // c[3] for c in EDGE_CASES} == {1, 3, 4, 8}
    assert any(c[1] == 2048 and c[2] // c[3] == 8 for c in CASES)
    assert any(0 in c[4] for c in CASES)
    assert any(n % KC == 0 and 0 < n < c[1] for c in CASES for n in c[4])        # kv_len exactly on a key-chunk edge
    assert any(n % KC == 1 and n > 1 for c in CASES for n in c[4])               # ... and one past it
    assert any(0 < n < KC and c[1] > 2 * KC + QC for c in CASES for n in c[4])   # whole padded query chunks attend chunk 0 only
    assert any(L % 32 == 1 for L in Ls) and any(c[1] % 32 == 0 and any(n % 32 == 31 for n in c[4]) for c in CASES)
    assert {c[1] for c in BOTH_ENTRIES} == {300, 544}
    assert ADVERSARY_CASE[:4] == (1, 1040, 4, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# launching

class Launch:
    """One tcavt_attn_causal_gqa_stream call with out and lse inside NaN-filled buffers (fwd.Launch for the stream entry)"""

    def __init__(self, qkv, kv_len, B, L, nq, nkv, with_lse=True):
        capi = fwd._lib()
        dev, dt = qkv.device, qkv.dtype
        n, W, G = B * L, nq * 64, fwd._GUARD
        self.ob = torch.full((n + 2 * G, W), float("nan"), dtype=dt, device=dev)
        self.lb = torch.full((B * nq * L + 128,), float("nan"), dtype=F32, device=dev)
        ob0, lb0 = self.ob.clone(), self.lb.clone()
        self.out = self.ob[G:G + n]
        self.lse = self.lb[64:64 + B * nq * L].view(B, nq, L)
        self.rc = capi.lib().tcavt_attn_causal_gqa_stream(qkv.data_ptr(), self.out.data_ptr(), self.lse.data_ptr() if with_lse else None,
                                                          kv_len.data_ptr(), B, L, nq, nkv, SCALE, fwd._dt_code(dt), capi.stream_ptr())
        torch.cuda.synchronize()
        self.guards_ok = (torch.equal(_bits(self.ob[:G]), _bits(ob0[:G])) and torch.equal(_bits(self.ob[G + n:]), _bits(ob0[G + n:]))
                          and torch.equal(_bits(self.lb[:64]), _bits(lb0[:64]))
                          and torch.equal(_bits(self.lb[64 + B * nq * L:]), _bits(lb0[64 + B * nq * L:])))
        self.lse_untouched = torch.equal(_bits(self.lb), _bits(lb0))


def _run_checked(qkv, kv_len, B, L, nq, nkv, what):
    """with lse (twice) and without: guards, finiteness, unchanged inputs, bit identity.  -> (out [B * L, nq * 64], lse [B, nq, L])"""
    capi = fwd._lib()
    buf = fwd._with_guard_rows(qkv)
    keep, keep_kv = buf.clone(), kv_len.clone()
    a = Launch(buf, kv_len, B, L, nq, nkv)
    capi.check(a.rc, what)
    assert a.guards_ok, f"{what}: write outside out / lse"
    assert torch.isfinite(a.out).all(), f"{what}: {int((~torch.isfinite(a.out)).sum())} non-finite (unwritten) out elements"
    assert torch.isfinite(a.lse).all(), f"{what}: {int((~torch.isfinite(a.lse)).sum())} non-finite (unwritten) lse elements"
    b = Launch(buf, kv_len, B, L, nq, nkv)
    c = Launch(buf, kv_len, B, L, nq, nkv, with_lse=False)
    for o, nm in ((b, "second launch"), (c, "lse == NULL")):
        capi.check(o.rc, f"{what} {nm}")
        assert o.guards_ok, f"{what} {nm}: write outside out / lse"
        assert torch.equal(_bits(o.out), _bits(a.out)), f"{what}: out of the {nm} call differs"
    assert torch.equal(_bits(b.lse), _bits(a.lse)), f"{what}: lse differs between two launches"
    assert c.lse_untouched, f"{what}: lse written by a call without lse"
    assert torch.equal(_bits(buf), _bits(keep)) and torch.equal(kv_len, keep_kv), f"{what}: qkv / kv_len modified"
    return a.out, a.lse


def _key(case, dt):
    return f"stream {_name(dt)} group {case[2] // case[3]}"


# ---------------------------------------------------------------------------------------------------------------------------
# planted codes at long lengths

def _far_codes(n, g, draw=fwd._codes):
    """fwd._codes with rejection: +-1 codes whose pairwise dots stay <= 40 (a row that is too close to an earlier one is
    drawn again)"""
    c = draw(n, g)
    for _ in range(64):
        d = c @ c.T
        close = (torch.triu(d, 1) > 40).any(0).nonzero().flatten()
        if close.numel() == 0:
            return c
        c[close] = draw(close.numel(), g)
    raise AssertionError("rejection sampling of the planted codes did not converge")


@contextlib.contextmanager
def _rejection_codes():
    keep = fwd._codes
    fwd._codes = _far_codes
    try:
        yield
    finally:
        fwd._codes = keep


def _planted(case, ci, dt, dev):
    with _rejection_codes():
        return fwd._planted(case, ci, dt, dev)  # (asserts dot <= 40 on the CPU itself)


def test_far_codes_keep_the_margin():
    g = torch.Generator().manual_seed(5)
    c = _far_codes(2048, g)
    d = c @ c.T
    d.fill_diagonal_(-64)
    assert d.max().item() <= 40 and bool((c.abs() == 1).all())
    assert fwd._codes is not _far_codes  # (the swap is undone)


# ---------------------------------------------------------------------------------------------------------------------------
# the two regimes

@gpu_test
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("ci", range(len(ALL_CASES)), ids=[f"{i}-{_case_id(c)}" for i, c in enumerate(ALL_CASES)])
def test_stream_planted(gpu, ci, dt):
    """out == V[t(i)] bit for bit; lse within 8 fp32 ulps of 512; a sample without a key gives exact zeros"""
    case = ALL_CASES[ci]
    B, L, nq, nkv, kv = case
    dev = gpu["device"]
    what = f"planted {_key(case, dt)}: {case}"
    qkv, tgt = _planted(case, ci, dt, dev)
    kv_len = torch.tensor(kv, dtype=torch.int32, device=dev)
    out, lse = _run_checked(qkv, kv_len, B, L, nq, nkv, what)
    x = qkv.view(B, L, nq + 2 * nkv, 64)
    vh = x[:, :, nq + nkv:].repeat_interleave(nq // nkv, dim=2)
    want = torch.gather(vh, 1, tgt.clamp_min(0)[..., None].expand(B, L, nq, 64))
    want = torch.where((tgt >= 0)[..., None], want, torch.zeros((), dtype=dt, device=dev))
    bad = _bits(out.view(B, L, nq, 64)) != _bits(want.contiguous())
    if bool(bad.any()):
        b, i, h, d = fwd._first_bad(bad)
        raise AssertionError(f"{what}: {int(bad.any(-1).sum())} rows are not V[target]; first: sample {b} query {i} head {h} target "
                             f"{int(tgt[b, i, h])} kv_len {kv[b]}: got key (tile, offset) = {out.view(B, L, nq, 64)[b, i, h, :2].tolist()}")
    has = (tgt >= 0).permute(0, 2, 1)
    exp_lse = torch.where(has, 512.0, 0.0).double()
    d = (lse.double() - exp_lse).abs()
    assert bool((d <= 8 * 2.0 ** -14).all()), f"{what}: lse off 512 by {d.max().item():.3e} (8 ulp = 4.9e-4)"
    fwd._check_empty_samples(out, lse, kv, B, L, nq, what)
    if ci < len(CASES):  # the float64 reference agrees with the construction
        ref, lse_ref, _, _, _ = fwd._attn_ref(qkv, kv_len, B, L, nq, nkv)
        assert torch.equal(ref.float().to(dt), want.view(B * L, nq * 64)), "the planted construction is not exact in float64"
        assert bool(((lse_ref - exp_lse).abs() < 1e-9).all())


def _check_realistic(out, lse, qkv, kv_len, case, dt, what, key, refs=None):
    B, L, nq, nkv, kv = case
    ref, lse_ref, pav, sav, nat = refs if refs is not None else fwd._attn_ref(qkv, kv_len, B, L, nq, nkv)
    fwd._check_single_key_rows(out, qkv, nat, B, L, nq, nkv, what)
    fwd._check_empty_samples(out, lse, kv, B, L, nq, what)
    fwd._check_bound(out, ref, pav, sav, dt, what, key)
    fwd._check_global(out, ref, dt, what, key)
    fwd._check_lse(lse, lse_ref, what, key)


@gpu_test
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("ci", range(len(ALL_CASES)), ids=[f"{i}-{_case_id(c)}" for i, c in enumerate(ALL_CASES)])
def test_stream_realistic(gpu, ci, dt):
    case = ALL_CASES[ci]
    B, L, nq, nkv, kv = case
    dev = gpu["device"]
    what = f"real {_key(case, dt)}: {case}"
    qkv = fwd._realistic(case, ci, dt, dev)
    kv_len = torch.tensor(kv, dtype=torch.int32, device=dev)
    out, lse = _run_checked(qkv, kv_len, B, L, nq, nkv, what)
    _check_realistic(out, lse, qkv, kv_len, case, dt, what, _key(case, dt))


@gpu_test
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", BOTH_ENTRIES, ids=_case_id)
def test_stream_and_resident_meet_the_same_bound(gpu, case, dt):
    """L <= 544: both entries against float64 on the same inputs (bit equality between them is not required)"""
    B, L, nq, nkv, kv = case
    dev = gpu["device"]
    qkv = fwd._realistic(case, L, dt, dev)
    kv_len = torch.tensor(kv, dtype=torch.int32, device=dev)
    refs = fwd._attn_ref(qkv, kv_len, B, L, nq, nkv)
    out_s, lse_s = _run_checked(qkv, kv_len, B, L, nq, nkv, f"stream {case}")
    out_r, lse_r = fwd._run_checked(qkv, kv_len, B, L, nq, nkv, f"resident {case}")
    _check_realistic(out_s, lse_s, qkv, kv_len, case, dt, f"real stream {_name(dt)}: {case}", _key(case, dt), refs)
    _check_realistic(out_r, lse_r, qkv, kv_len, case, dt, f"real resident {_name(dt)}: {case}", "resident beside " + _key(case, dt), refs)
    print(f"stream vs resident {case} {_name(dt)}: bit-equal out {torch.equal(_bits(out_s), _bits(out_r))}, lse {torch.equal(_bits(lse_s), _bits(lse_r))}")


@gpu_test
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_stream_adversaries(gpu, dt):
    """score patterns that stress the online softmax across key chunks, under the bound of the realistic regime"""
    case = ADVERSARY_CASE
    B, L, nq, nkv, kv = case
    dev = gpu["device"]
    kv_len = torch.tensor(kv, dtype=torch.int32, device=dev)
    for kind in ("increasing", "decreasing", "spike", "zero_q"):
        key = _key(case, dt) + " adversary"
        what = f"{kind} {key}: {case}"
        qkv = fwd._adversary(kind, case, dt, dev)
        out, lse = _run_checked(qkv, kv_len, B, L, nq, nkv, what)
        ref, lse_ref, pav, sav, nat = fwd._attn_ref(qkv, kv_len, B, L, nq, nkv)
        if kind == "decreasing":
            x = qkv.double().view(B, L, nq + 2 * nkv, 64)
            s = SCALE * (x[0, L - 1, 0] @ x[0, :, nq].T)
            assert (s[0] - s[kv[0] - 1]).item() > 17.0
        if kind == "zero_q":
            assert bool(((lse_ref - torch.log(nat.double())[:, None, :]).abs() < 1e-12).all())
        fwd._check_single_key_rows(out, qkv, nat, B, L, nq, nkv, what)
        fwd._check_bound(out, ref, pav, sav, dt, what, key)
        fwd._check_global(out, ref, dt, what, key, enforce=False)
        fwd._check_lse(lse, lse_ref, what, key)


@gpu_test
def test_stream_refusals(gpu):
    """bad arguments: non-zero status, a message that starts with the entry's name, out and lse untouched"""
    dev = gpu["device"]
    capi = fwd._lib()

    def call(B, L, nq, nkv, dt_code=None, shift_qkv=0, shift_out=0, alloc_L=64):
        aL = alloc_L
        qkv = torch.randn(B * aL * (nq + 2 * nkv) * 64 + 8, device=dev).to(F16)
        ob = torch.full((B * aL * nq * 64 + 8 + 1024,), float("nan"), dtype=F16, device=dev)
        lb = torch.full((B * nq * aL + 64,), float("nan"), dtype=F32, device=dev)
        ob0, lb0 = ob.clone(), lb.clone()
        kv_len = torch.full((B,), min(L, aL), dtype=torch.int32, device=dev)
        rc = capi.lib().tcavt_attn_causal_gqa_stream(qkv.data_ptr() + 2 * shift_qkv, ob.data_ptr() + 2 * shift_out, lb.data_ptr(),
                                                     kv_len.data_ptr(), B, L, nq, nkv, SCALE, capi.F16 if dt_code is None else dt_code,
                                                     capi.stream_ptr())
        torch.cuda.synchronize()
        return rc, torch.equal(_bits(ob), _bits(ob0)) and torch.equal(_bits(lb), _bits(lb0))

    rc, clean = call(2, 64, 4, 1)
    assert rc == 0 and not clean  # the harness itself: a good call is accepted and writes
    for name, kw in (("L = 0", dict(B=1, L=0, nq=4, nkv=1)), ("L = 2049", dict(B=1, L=2049, nq=4, nkv=1)),
                     ("group 9", dict(B=1, L=64, nq=9, nkv=1)), ("nq % nkv", dict(B=1, L=64, nq=5, nkv=2)),
                     ("f32", dict(B=1, L=64, nq=4, nkv=1, dt_code=capi.F32)),
                     ("unaligned qkv", dict(B=1, L=64, nq=4, nkv=1, shift_qkv=1)),
                     ("unaligned out", dict(B=1, L=64, nq=4, nkv=1, shift_out=1))):
        capi.lib().tcavt_attn_causal_gqa_stream(None, None, None, None, 1, 1, 1, 1, SCALE, capi.F16, capi.stream_ptr())
        assert "null pointer" in fwd._last_error()
        rc, clean = call(**kw)
        assert rc != 0, f"{name}: accepted"
        assert fwd._last_error().startswith("attn_causal_gqa_stream:") and "null pointer" not in fwd._last_error(), f"{name}: {fwd._last_error()!r}"
        assert clean, f"{name}: a refused call wrote"
    # the resident entry still refuses what the stream entry takes
    qkv = torch.zeros(545 * 6 * 64, dtype=F16, device=dev)
    out = torch.full((545 * 4 * 64,), float("nan"), dtype=F16, device=dev)
    kv_len = torch.full((1,), 545, dtype=torch.int32, device=dev)
    rc = capi.lib().tcavt_attn_causal_gqa_lse(qkv.data_ptr(), out.data_ptr(), None, kv_len.data_ptr(), 1, 545, 4, 1, SCALE, capi.F16,
                                              capi.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and bool(torch.isnan(out).all())


@gpu_test
def test_report_worst_ratio(gpu):
    """(runs last in file order) prints the worst ratios measured in this session per instantiation (type) and group"""
    for k in sorted(k for k in fwd._WORST_C if "stream" in k):
        print(f"attn  {k:44s} worst c {fwd._WORST_C[k]:7.3f}   worst r {fwd._WORST_R.get(k, 0.0):6.3f}   lse {fwd._WORST_LSE.get(k, 0.0):5.2f} ulp")
