"""The chunked attention backward beyond 544 rows (tcavt_attn_bwd_stream: attn_bwd_dq_long_kernel<U> + attn_bwd_dkv_long_kernel
under the cap of the streaming forward, 2048) against float64.

The reference, the planted and realistic regimes, the NaN-guarded buffers, the bound and its bars (_C, _R, the _U / _E units)
are those test_attention_bwd_gpu.py applies to tcavt_attn_bwd_long (imported, not copied).  The fp32 accumulation term of that
bound carries the number of summed terms (T for dQ, T * group for dK / dV) and is evaluated here at the T of the case.  The
absolute bars against fp32 autograd are ABS_BAR of test_attn_bwd_long_gpu.py.

Cases (B, T, nq, nkv, kv_len), each in fp16 and bf16; (QC, query chunks, key chunks) by the host rule (_long_chunks):

| case | group | chunks | why |
|---|---|---|---|
| (2, 545, 4, 1, [545, 512]) | 4 | (128, 5, 3) | first length past tcavt_attn_bwd_long; third key chunk of 33 keys; kv_len on a chunk edge |
| (2, 800, 2, 2, [800, 0]) | 1 | (256, 4, 4) | U = 1; a sample without keys; last chunk partial (32 of 256) |
| (2, 1040, 8, 2, [1040, 700]) | 4 | (128, 9, 5) | stage 1's length; last query chunk of 16 rows: one strip pair, the rest beyond T |
| (1, 1040, 16, 1, [1024]) | 16 | (32, 33, 5) | group 16; kv_len on a chunk edge, 16 padded queries behind it |
| (1, 2048, 4, 4, [2048]) | 1 | (256, 8, 8) | the cap; eight chunks both ways |
| (1, 2048, 8, 2, [1500]) | 4 | (128, 16, 8) | the cap; two whole key chunks behind kv_len |
| (1, 2048, 16, 1, [2048]) | 16 | (32, 64, 8) | the cap at group 16: B nq T = 32768 rows of stats |

Planted codes are drawn with rejection at these lengths (the setup's `dot <= 40` assertion stays; see the forward file).
At T = 544 the stream entry and tcavt_attn_bwd_long both meet the bound on the same inputs.
Measured worst ratios: profiles/attention_stream_bounds.txt; test_report_worst_ratio prints this session's (pytest -s).
"""
import contextlib

import pytest
import torch

import test_attention_bwd_gpu as bwd
from test_attention_bwd_gpu import BF16, DTYPES, F16, _C, _case_id, _name, _same_bits
from test_attn_bwd_long_gpu import ABS_BAR

gpu_test = pytest.mark.gpu

STREAM_CASES = [
    (2, 545, 4, 1, [545, 512]),
    (2, 800, 2, 2, [800, 0]),
    (2, 1040, 8, 2, [1040, 700]),
    (1, 1040, 16, 1, [1024]),
    (1, 2048, 4, 4, [2048]),
    (1, 2048, 8, 2, [1500]),
    (1, 2048, 16, 1, [2048]),
]
AT_544 = (2, 544, 4, 1, [544, 513])
ADVERSARY_CASE = (1, 1040, 4, 1, [1040])


def _kernels(case):
    return [f"attn_bwd_dq_long_kernel<U={min(case[2] // case[3], 2)}>", "attn_bwd_dkv_long_kernel"]


def _key(case, dt, extra=""):
    return ("tcavt_attn_bwd_stream", " + ".join(_kernels(case)) + extra, _name(dt))


def test_paths_coverage():
    """from the list alone (no GPU): the lengths, groups and kv_len patterns asked for, both dQ instantiations, and the host
    rule's chunk counts up to the cap"""
    Ts = {c[1] for c in STREAM_CASES}
    assert Ts == {545, 800, 1040, 2048}
    for B, T, nq, nkv, kv in STREAM_CASES + [AT_544, ADVERSARY_CASE]:
        assert 1 <= B <= 3 and nq <= 16 and len(kv) == B and all(0 <= n <= T for n in kv) and 16 % (nq // nkv) == 0
    assert {c[2] // c[3] for c in STREAM_CASES} == {1, 4, 16}
    assert {c[2] // c[3] for c in STREAM_CASES if c[1] == 2048} == {1, 4, 16}
    assert {k for c in STREAM_CASES for k in _kernels(c)} == {"attn_bwd_dq_long_kernel<U=1>", "attn_bwd_dq_long_kernel<U=2>",
                                                              "attn_bwd_dkv_long_kernel"}
    assert any(0 in c[4] for c in STREAM_CASES)
    assert any(n % 256 == 0 and 0 < n < c[1] for c in STREAM_CASES for n in c[4])  # kv_len on a chunk edge
    assert any(max(c[4]) + 256 < c[1] for c in STREAM_CASES)                       # whole key chunks behind kv_len
    assert any(min(c[4]) < c[1] for c in STREAM_CASES) and any(len(set(c[4])) == 2 for c in STREAM_CASES)  # ragged
    assert bwd._long_chunks(545, 4, 1) == (128, 5, 3) and bwd._long_chunks(1040, 8, 2) == (128, 9, 5)
    assert bwd._long_chunks(1040, 16, 1) == (32, 33, 5) and bwd._long_chunks(2048, 16, 1) == (32, 64, 8)
    assert bwd._long_chunks(2048, 4, 4) == (256, 8, 8) and bwd._long_chunks(800, 2, 2) == (256, 4, 4)
    assert {bwd._long_chunks(c[1], c[2], c[3])[2] for c in STREAM_CASES} >= {3, 4, 5, 8}  # 5 to 8 key chunks among them
    assert AT_544[1] == 544


# ---------------------------------------------------------------------------------------------------------------------------
# planted codes at long lengths; realistic inputs shared between the tests

def _far_codes(n, g, draw=bwd._codes):
    c = draw(n, g)
    for _ in range(64):
        close = (torch.triu(c @ c.T, 1) > 40).any(0).nonzero().flatten()
        if close.numel() == 0:
            return c
        c[close] = draw(close.numel(), g)
    raise AssertionError("rejection sampling of the planted codes did not converge")


@contextlib.contextmanager
def _rejection_codes():
    keep = bwd._codes
    bwd._codes = _far_codes
    try:
        yield
    finally:
        bwd._codes = keep


def _planted(case, ci, dt, dev):
    with _rejection_codes():
        return bwd._planted(case, ci, dt, dev)  # (asserts dot <= 40 on the CPU itself)


@gpu_test
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("case", STREAM_CASES, ids=_case_id)
def test_stream_planted(gpu, case, dt):
    dev = gpu["device"]
    what = f"planted stream {_name(dt)}: {case}"
    inp, dv_want, delta = _planted(case, 100 + STREAM_CASES.index(case), dt, dev)
    g, stats = bwd._two_launch("stream", inp, what)
    bwd._check_planted(g, stats, inp, dv_want, delta, dt, what, rotated=True)


@gpu_test
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("case", STREAM_CASES, ids=_case_id)
def test_stream_realistic(gpu, case, dt):
    """the float64 bound per element and per block; every element written with NaN rows behind the inputs; a second launch
    (zero rows behind the inputs) bit-equal; the absolute bar against fp32 autograd"""
    import test_attn_bwd_long_gpu as long_gpu
    from tests.util import rel_err

    dev = gpu["device"]
    B, T, nq, nkv, kv = case
    key = _key(case, dt)
    what = f"real stream {_name(dt)}: {case}"
    inp, ref = bwd._real_case(case, dt, dev)
    g, stats = bwd._two_launch("stream", inp, what)
    bwd._check_stats_lse(stats, ref, inp, what)
    bwd._check_empty_samples(g, inp, what)
    bwd._check_g16(g, ref, inp, _C, what, key)
    g2, stats2 = bwd._two_launch("stream", inp, what + " (second launch, zero rows behind the inputs)", fill=0.0)
    assert _same_bits(g2, g) and _same_bits(stats2, stats), f"{what}: two launches differ"
    # fp32 autograd + rope_bwd_pack, the absolute bars of the chunked form (a sample without keys has no softmax to differentiate)
    if min(kv) > 0:
        from tcavt_amd import ops

        want32, _, _ = long_gpu._attn_ref(inp.qkv, inp.dO, inp.kv_len, B, T, nq, nkv)
        want = torch.empty(B * T, inp.ncols, dtype=dt, device=dev)
        ops.rope_bwd_pack(want32.contiguous(), want, inp.cos, inp.sin, (nq + nkv) * 64, T)
        for name, lo, hi in bwd._blocks(nq, nkv):
            e = rel_err(g[:, lo:hi].float().cpu(), want[:, lo:hi].float().cpu())
            print(f"[attn_bwd_stream {case} {_name(dt)}] {name}: {e:.3e} against fp32 autograd")
            assert e < ABS_BAR[dt], (name, e)


@gpu_test
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_stream_and_long_agree_at_544(gpu, dt):
    """T = 544 through both entries on the same inputs: each within the float64 bound (today they are the same two launches,
    so the bits agree as well; that is printed, the bound is what is asserted)"""
    dev = gpu["device"]
    case = AT_544
    inp, ref = bwd._real_case(case, dt, dev)
    g_s, st_s = bwd._two_launch("stream", inp, f"stream at 544 {_name(dt)}")
    g_l, st_l = bwd._two_launch("long", inp, f"long at 544 {_name(dt)}")
    bwd._check_g16(g_s, ref, inp, _C, f"real stream {_name(dt)}: {case}", _key(case, dt, " at 544"))
    bwd._check_g16(g_l, ref, inp, _C, f"real long {_name(dt)}: {case}", ("tcavt_attn_bwd_long", "beside the stream entry at 544", _name(dt)))
    assert _same_bits(st_s, st_l), "stats differ between the two entries"
    print(f"stream vs long at 544 {_name(dt)}: bit-equal {_same_bits(g_s, g_l)}")


@gpu_test
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_stream_adversaries(gpu, dt):
    dev = gpu["device"]
    case = ADVERSARY_CASE
    for kind in ("increasing", "decreasing", "spike", "zero_q"):
        key = _key(case, dt, " adversary")
        what = f"{kind} stream {_name(dt)}: {case}"
        inp = bwd._adversary(kind, case, dt, dev)
        ref = bwd.Ref(inp, True, dt)
        g, stats = bwd._two_launch("stream", inp, what)
        bwd._check_stats_lse(stats, ref, inp, what)
        bwd._check_g16(g, ref, inp, _C, what, key)


@gpu_test
def test_composition_takes_the_stream_form_and_the_switch_the_tiled_one(gpu, monkeypatch):
    """llm_backward.attn_bwd_composed at T = 545: the third branch; behind TCAVT_ATTN_BWD_NO_STREAM the tiled kernels, which
    meet the same absolute bar against each other"""
    from tcavt_amd import ops
    from tcavt_amd.llm_backward import attn_bwd_composed
    from tests.util import rel_err

    dev = gpu["device"]
    case = STREAM_CASES[0]
    B, T, nq, nkv, kv = case
    inp, _ = bwd._real_case(case, F16, dev)
    pool = {}

    def buf(name, shp, dtype, zero=False):
        if name not in pool:
            pool[name] = torch.zeros(shp, dtype=dtype, device=dev)
        return pool[name]

    calls = []
    real = ops.attn_bwd_stream
    monkeypatch.setattr(ops, "attn_bwd_stream", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    qkv_p, dO_p, att_p = inp.padded(64, 0.0)
    via, tiled = torch.empty_like(inp.qkv), torch.empty_like(inp.qkv)
    attn_bwd_composed(buf, qkv_p, dO_p[:B * T], inp.kv_len, B, T, nq, nkv, 0.125, inp.cos, inp.sin, via, lse=inp.lse, att=att_p[:B * T])
    assert calls == [1], "attn_bwd_composed must take the stream form at T = 545"
    monkeypatch.setenv("TCAVT_ATTN_BWD_NO_STREAM", "1")
    attn_bwd_composed(buf, qkv_p, dO_p[:B * T], inp.kv_len, B, T, nq, nkv, 0.125, inp.cos, inp.sin, tiled, lse=inp.lse, att=att_p[:B * T])
    torch.cuda.synchronize()
    assert calls == [1]
    g, _ = bwd._two_launch("stream", inp, "direct")
    assert _same_bits(via, g)
    for name, lo, hi in bwd._blocks(nq, nkv):
        e = rel_err(via[:, lo:hi].float().cpu(), tiled[:, lo:hi].float().cpu())
        print(f"[composition T=545] {name}: stream vs tiled {e:.3e}")
        assert e < ABS_BAR[F16], (name, e)


@gpu_test
def test_report_worst_ratio(gpu):
    """(runs last in file order) prints the worst ratios measured in this session per (entry, kernels, type)"""
    for k in sorted(k for k in bwd._WORST if "stream" in k[0] or "stream" in k[1]):
        w = bwd._WORST[k]
        print(f"{k[0]:24s} {k[1]:62s} {k[2]:5s} worst c {w.get('c', 0.0):6.3f}  worst r {w.get('r', 0.0):6.3f}  of the bound {w.get('frac', 0.0):6.3f}")
