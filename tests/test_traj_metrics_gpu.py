"""tcavt_traj_metrics (csrc/small.hip) against float64, called on its own: the loss numerators sums[0..1], the metric sums
sums[2..4], per_sample, the three argmins, argmin == NULL / per_sample == NULL, accumulation over calls.

Every case calls the C entry point (capi.lib().tcavt_traj_metrics) and checks every value against ONE float64 evaluation of the
header's formula in torch on the CPU, from the same fp32 input values; nothing in a reference comes from a project kernel.  sums,
per_sample and argmin lie between guard rows (NaN, for argmin a sentinel), pred / gt / norm_stat have NaN rows behind them: every
guard keeps its bits, every input stays bit-unchanged, a second launch from the same start gives the same bits.

sums[0..1] at K > 1 are those of candidate k = 0 (the kernel keeps sx, sy of k == 0; model.py forms the loss from them with
K = 1), and are checked as such at every shape.

| shape (B, K, To) | why |
|---|---|
| (1, 1, 1) | smallest: 15 idle waves, one lane |
| (3, 2, 5) | small, K > 1 |
| (16, 10, 30) | one sample per wave |
| (17, 10, 64) | wave 0 takes two samples; To fills the 64 lanes exactly |
| (37, 10, 65) | three samples on waves 0..4; a second lane round with one element |
| (33, 3, 130) | three lane rounds; three samples on wave 0 alone |

norm_stat: pixel-scale ranges up to 3839 (x) and 2159 (y), different per sample.  K >= 8: candidates 3 and 7 are exact
duplicates and, on every even sample, by far the best (ADE, RMSE; FDE on most of them): the first index must win.

Regimes:
- realistic: pred = gt + 0.05 randn; bound derived in _reference from the kernel's operation chain (bar 1.0); the argmins are
  asserted exactly, after asserting on the float64 values alone that best and second-best distinct value lie further apart than
  twice the bound.
- integer: norm_stat = (0, r, 0, r), r a power of two, pred and gt multiples of 1 / r: every dx, dy is a small integer, every
  sum stays below 2^24 (asserted), sums[0..1] must equal the float64 sums bit for bit.
- non-finite: one NaN / one +inf in pred of candidate 0 makes sums[0] / sums[1] non-finite (tcavt_adamw_gated's gate lives on
  that); the other samples' per_sample rows stay finite and inside their bounds.

Refusals pass only arguments that the host code rejects before any launch (NULL pointers, B, K or To = 0).

MEASURED on an MI355X: the worst fraction of the bound stands beside the constants below; profiles/fp32_train_tail_bounds.txt
has every line and the mutants, test_report_worst_ratio prints the session's values (pytest -s).
"""
import pytest
import torch

from test_attention_bwd_gpu import _first_bad, _same_bits
from test_forward_row_kernels_gpu import _guarded, _refused
from test_gemm_forms_gpu import _ulp
from test_head_forward_kernels_gpu import _dev, _ins, _p
from test_llm_backward_kernels_gpu import _gen, _L, _ok, _st, _unchanged

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
_E = 2.0 ** -24   # unit roundoff of fp32
_WAVES, _LANES = 16, 64                     # traj_metrics_kernel: ONE workgroup of 1024 threads
# MEASURED on an MI355X: worst fraction of the whole bound (bar 1.0) over the realistic cases
#   per_sample ADE 0.055   FDE 0.315   RMSE 0.085
#   sums[0..1]     0.122   sums[2..4]  0.060   (accumulated over two calls: 0.033)
# Mutants (profiles/fp32_train_tail_bounds.txt): FDE at To - 2, RMSE divided by To, the sample loop without its stride, <= in
# the argmin, sums[i] = t: each fails here; the earlier test passes `sums[i] = t`.
_WORST = {}

SHAPES = [(1, 1, 1), (3, 2, 5), (16, 10, 30), (17, 10, 64), (37, 10, 65), (33, 3, 130)]
_DUP = (3, 7)   # K >= 8: candidate 7 is a copy of candidate 3


def _per_wave(B):
    """samples of wave w: w, w + 16, ..."""
    return [len(range(w, B, _WAVES)) for w in range(_WAVES)]


def _rounds(To):
    """(iterations of the lane loop `for t = lane; t < To; t += 64` on lane 0, elements in the last round)"""
    return -(-To // _LANES), (To - 1) % _LANES + 1


def test_cases_cover_the_host_rules():
    """from the case list alone (the launch arithmetic of the entry point mirrored: one workgroup, 16 waves, wave w takes samples
    w, w + 16, ..., lanes over time steps in rounds of 64): every path and edge is reached"""
    pw = {s: _per_wave(s[0]) for s in SHAPES}
    assert SHAPES[0] == (1, 1, 1) and pw[SHAPES[0]].count(0) == 15
    assert any(B < _WAVES and K > 1 for B, K, _ in SHAPES)                                        # idle waves with K > 1
    assert any(set(v) == {1} for v in pw.values())                                                # one sample per wave
    assert any(sorted(set(v)) == [1, 2] and v.count(2) == 1 for v in pw.values())                 # one wave takes two
    assert any(max(v) == 3 and v.count(3) > 1 for v in pw.values()) and any(max(v) == 3 and v.count(3) == 1 for v in pw.values())
    assert any(B > 32 for B, _, _ in SHAPES)
    r = [_rounds(To) for _, _, To in SHAPES]
    assert (1, 1) in r and (1, 64) in r and (2, 1) in r and any(n == 3 and 1 < last < 64 for n, last in r)
    assert any(K == 1 for _, K, _ in SHAPES) and sum(K >= 8 for _, K, _ in SHAPES) >= 3 and all(K > max(_DUP) for _, K, _ in SHAPES if K >= 8)


# ---------------------------------------------------------------------------------------------------------------------------
# data, reference and bound

def _batch(B, K, To, seed):
    """float64 on the CPU (values of fp32): gt in [0, 1), pred = gt + 0.05 randn, norm_stat with pixel-scale ranges"""
    g_ = _gen(seed)
    gt = torch.rand(B, 2, To, generator=g_)
    pred = gt[:, None] + 0.05 * torch.randn(B, K, 2, To, generator=g_)
    if K >= 8:
        pred[0::2, _DUP[0]] = gt[0::2] + 0.005 * torch.randn(gt[0::2].shape, generator=g_)
        pred[:, _DUP[1]] = pred[:, _DUP[0]]
    b = torch.arange(B, dtype=F32)
    minx, miny = torch.floor(torch.rand(B, generator=g_) * 900), torch.floor(torch.rand(B, generator=g_) * 500)
    maxx, maxy = 3839.0 - 7 * b - torch.floor(torch.rand(B, generator=g_) * 600), 2159.0 - 3 * b - torch.floor(torch.rand(B, generator=g_) * 400)
    ns = torch.stack([minx, maxx, miny, maxy], dim=1)
    assert bool((ns[:, 1] - ns[:, 0] > 1000).all()) and ns.max().item() <= 3839 and len({tuple(r) for r in ns.tolist()}) == B
    return pred.float(), gt.float(), ns.float()


def _int_batch(B, K, To, seed):
    """norm_stat = (0, r, 0, r), r a power of two; pred, gt multiples of 1 / r: every dx, dy an integer in [-12, 12]"""
    g_ = _gen(seed)
    r = torch.ldexp(torch.ones(B), torch.randint(6, 12, (B,), generator=g_))
    gt = torch.randint(0, 7, (B, 2, To), generator=g_).float() / r[:, None, None]
    pred = torch.randint(-6, 13, (B, K, 2, To), generator=g_).float() / r[:, None, None, None]
    z = torch.zeros(B)
    return pred, gt, torch.stack([z, r, z, r], dim=1)


def _reference(pred, gt, ns):
    """float64 values and per-value fp32 bounds, from the chain of traj_metrics_kernel (-ffp-contract=off: every operation rounds
    once, E = 2^-24):
      rx = max - min; dn = p * rx + min: three roundings (rx, the product, the sum), each at most E (|p r| + |min|)
      dx = dn_p - dn_g:   Ex = 3 E (|p r| + |min|) + 3 E (|g r| + |min|) + E |dx|      -- the cancellation: Ex stays at the scale
                          of the de-normalised values, |dx| is ~50 times smaller
      dx * dx:            2 |dx| Ex + Ex^2 + E dx^2
      err = sqrtf(dx^2 + dy^2): the norm of (dx, dy) moves by at most Ex + Ey; the two products, the sum and the square root
                          add 3 E err (half of 2 E on the radicand, 2 E on sqrtf)
      lane sums:          ceil(To / 64) serial additions, then 6 exchange levels: nred E (sum)
      ade = se / To:      mean of the err bounds + (nred + 1) E ade;    fde = err[To - 1] through exact additions of zeros
      rmse = sqrtf((sx + sy) / (2 To)):  q moves by dq = (dsx + dsy + E (sx + sy)) / (2 To) + E q; rmse by dq / (2 rmse) + 2 E rmse
      min over k:         by at most the largest bound among the candidates
    Returns dict of [B] tensors (ade, fde, rmse: min over k; sx, sy: candidate 0), their bounds d*, the [B, K] values and argmins."""
    B, K, _, To = pred.shape
    p, g, n = pred.double(), gt.double(), ns.double()
    mn, rg = n[:, [0, 2]], n[:, [1, 3]] - n[:, [0, 2]]                                   # [B, 2]
    pr, gr = p * rg[:, None, :, None], g * rg[:, :, None]
    d = (pr + mn[:, None, :, None]) - (gr + mn[:, :, None])[:, None]                     # [B, K, 2, To]
    Ed = 3 * _E * (pr.abs() + mn.abs()[:, None, :, None]) + 3 * _E * (gr.abs() + mn.abs()[:, :, None])[:, None] + _E * d.abs()
    sq = d * d
    dsq = 2 * d.abs() * Ed + Ed * Ed + _E * sq
    err = sq.sum(2).sqrt()                                                               # [B, K, To]
    derr = Ed.sum(2) + 3 * _E * err
    nred = _rounds(To)[0] + 6
    ade, fde = err.mean(-1), err[..., -1]
    dade, dfde = derr.mean(-1) + (nred + 1) * _E * ade, derr[..., -1]
    sx = sq.sum(-1)                                                                      # [B, K, 2]
    dsx = dsq.sum(-1) + nred * _E * sx
    q = sx.sum(-1) / (2 * To)
    dq = (dsx.sum(-1) + _E * sx.sum(-1)) / (2 * To) + _E * q
    rmse = q.sqrt()
    drmse = torch.where(q > 0, dq / (2 * rmse).clamp_min(1e-300), dq.sqrt()) + 2 * _E * rmse
    out = {"K": {"ade": ade, "fde": fde, "rmse": rmse}, "argmin": torch.stack([ade.argmin(1), fde.argmin(1), rmse.argmin(1)], 1)}
    for k, v, dv in (("ade", ade, dade), ("fde", fde, dfde), ("rmse", rmse, drmse)):
        out[k], out["d" + k] = v.min(1).values, dv.max(1).values
    out["sx"], out["sy"], out["dsx"], out["dsy"] = sx[:, 0, 0], sx[:, 0, 1], dsx[:, 0, 0], dsx[:, 0, 1]
    return out


_SUMS = ["sx", "sy", "ade", "fde", "rmse"]


def _sums_reference(ref, B, prev=None):
    """sums[i] = prev[i] + sum_b value_b: a wave adds its ceil(B / 16) samples, thread i the 16 waves' partials, then one += onto
    sums[i]: (ceil(B / 16) + 17) E (sum |value| + |prev|) on top of the samples' own bounds"""
    prev = torch.zeros(5, dtype=F64) if prev is None else prev
    tot = torch.stack([ref[k].sum() for k in _SUMS]) + prev
    n = max(_per_wave(B)) + _WAVES + 1
    f32 = torch.stack([ref["d" + k].sum() + n * _E * (ref[k].abs().sum()) for k in _SUMS]) + n * _E * prev.abs()
    return tot, f32


def _judge(got, ref, f32, what, key):
    """|got - ref| <= 1.01 * f32 + ulp_fp32(ref) per element, every element finite; records the worst fraction"""
    g = got.double().cpu().reshape(ref.shape)
    assert torch.isfinite(g).all(), f"{what}: {int((~torch.isfinite(g)).sum())} non-finite (unwritten?) values"
    bound = 1.01 * f32 + _ulp(ref, F32)
    d = (g - ref).abs()
    frac = (d / bound).max().item()
    _WORST[key] = max(_WORST.get(key, -1.0), frac)
    print(f"frac {what}: {frac:.3f}")
    bad = d > bound
    if bool(bad.any()):
        i = _first_bad(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} values out of bound (worst fraction {frac:.3f}); first {i}: "
                             f"got {g[i].item()!r} ref {ref[i].item()!r} allowed {bound[i].item():.3e}")


class _IntGuard:
    """argmin [B][3] int32 between four sentinel rows on each side"""
    FILL = -777

    def __init__(self, B, dev):
        self.buf = torch.full((B + 8, 3), self.FILL, dtype=torch.int32, device=dev)
        self.B, self.before = B, self.buf.clone()

    @property
    def region(self):
        return self.buf[4: 4 + self.B]

    @property
    def ptr(self):
        return self.region.data_ptr()

    def check(self, what):
        out = torch.ones_like(self.buf, dtype=torch.bool)
        out[4: 4 + self.B] = False
        assert torch.equal(self.buf[out], self.before[out]), f"{what}: write outside argmin[{self.B}][3]"


class _Inputs:
    def __init__(self, pred, gt, ns, dev):
        B, K, _, To = pred.shape
        self.B, self.K, self.To = B, K, To
        self.pred, self.gt, self.ns = _dev(pred.reshape(B * K * 2, To), dev), _dev(gt.reshape(B * 2, To), dev), _dev(ns, dev)
        self.ins = _ins(pred=self.pred, gt=self.gt, norm_stat=self.ns)


def _call(x, dev, what, start=None, outputs=True):
    """two launches from the same start into fresh guarded outputs: status, guards, inputs, reproducibility.
    Returns (sums, argmin, per_sample) of the first"""
    runs = []
    for tag in ("", " again"):
        sums = _guarded(1, 5, F32, dev, fill=torch.zeros(1, 5) if start is None else start.reshape(1, 5))
        am, per = (_IntGuard(x.B, dev), _guarded(x.B, 3, F32, dev)) if outputs else (None, None)
        _ok(_L().tcavt_traj_metrics(x.pred.buf.data_ptr(), x.gt.buf.data_ptr(), x.ns.buf.data_ptr(), sums.ptr, _p(am), _p(per),
                                    x.B, x.K, x.To, _st()), what + tag)
        for o in (sums, am, per):
            if o is not None:
                o.check(what + tag)
        _unchanged(x.ins, what + tag)
        runs.append((sums, am, per))
    for a, b in zip(*runs):
        assert a is None or torch.equal(a.region.view(torch.int32), b.region.view(torch.int32)), what + ": not reproducible"
    return runs[0]


def _assert_gaps(ref, what):
    """on the float64 values alone: per sample and metric, best and second-best DISTINCT value further apart than twice the bound
    (so that no in-bound fp32 evaluation can pick another candidate; exact duplicates tie in fp32 as well)"""
    worst = float("inf")
    for k in ("ade", "fde", "rmse"):
        for b, row in enumerate(ref["K"][k]):
            u = torch.unique(row)                      # sorted
            if len(u) > 1:
                bound = 1.01 * ref["d" + k][b] + _ulp(u[:1], F32)[0]
                worst = min(worst, ((u[1] - u[0]) / bound).item())
                assert u[1] - u[0] > 2 * bound, f"{what}: {k} of sample {b}: the two best values are {u[1] - u[0]:.3e} apart, bound {bound:.3e}: change the seed"
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# tests

@pytest.mark.parametrize("B,K,To", SHAPES)
def test_realistic(gpu, B, K, To):
    """per_sample, sums[0..4], argmins; the same sums bits with argmin and per_sample NULL"""
    dev = gpu["device"]
    pred, gt, ns = _batch(B, K, To, 1000 + B * K * To)
    x = _Inputs(pred, gt, ns, dev)
    ref = _reference(x.pred.region.cpu().view(B, K, 2, To), x.gt.region.cpu().view(B, 2, To), x.ns.region.cpu())
    what = f"traj_metrics {(B, K, To)}"
    gap = _assert_gaps(ref, what)
    print(f"{what}: nearest pair of candidates {gap:.0f} bounds apart")
    if K >= 8:
        even = ref["argmin"][0::2] == _DUP[0]        # (FDE is one time step: there another candidate may come nearer by chance)
        assert bool(even[:, [0, 2]].all()) and 2 * int(even[:, 1].sum()) > len(even), what + ": the duplicated candidate is not the best one on the even samples"
    sums, am, per = _call(x, dev, what)
    for i, k in enumerate(("ade", "fde", "rmse")):
        _judge(per.region[:, i], ref[k], ref["d" + k], f"{what} per_sample {k}", "per_sample " + k)
    tot, f32 = _sums_reference(ref, B)
    _judge(sums.region[0, :2], tot[:2], f32[:2], what + " sums[0..1]", "sums[0..1]")
    _judge(sums.region[0, 2:], tot[2:], f32[2:], what + " sums[2..4]", "sums[2..4]")
    got = am.region.cpu().long()
    assert torch.equal(got, ref["argmin"]), f"{what}: argmin differs at {_first_bad(got != ref['argmin'])}"
    s0, _, _ = _call(x, dev, what + " argmin = per_sample = NULL", outputs=False)
    assert _same_bits(s0.region, sums.region), what + ": sums differ without argmin and per_sample"


@pytest.mark.parametrize("B,K,To", SHAPES)
def test_accumulates_over_calls(gpu, B, K, To):
    """a second call, on another batch, onto the non-zero sums of the first: the accumulated float64 value"""
    dev = gpu["device"]
    xs, refs = [], []
    for seed in (2000, 3000):
        pred, gt, ns = _batch(B, K, To, seed + B * K * To)
        xs.append(_Inputs(pred, gt, ns, dev))
        refs.append(_reference(xs[-1].pred.region.cpu().view(B, K, 2, To), xs[-1].gt.region.cpu().view(B, 2, To), xs[-1].ns.region.cpu()))
    what = f"traj_metrics {(B, K, To)} second call"
    s1, _, _ = _call(xs[0], dev, what + " (first)")
    tot1, f1 = _sums_reference(refs[0], B)
    s2, _, _ = _call(xs[1], dev, what, start=s1.region.cpu())
    tot2, f2 = _sums_reference(refs[1], B, prev=tot1)
    assert bool((tot2 > tot1).all())                   # (the second batch counts)
    _judge(s2.region[0], tot2, f1 + f2, what, "sums accumulated")


@pytest.mark.parametrize("B,K,To", SHAPES)
def test_integer_sums_exact(gpu, B, K, To):
    """every dx, dy a small integer: sums[0..1] equal the float64 sums of candidate 0 bit for bit, from zero and accumulated"""
    dev = gpu["device"]
    pred, gt, ns = _int_batch(B, K, To, 4000 + B * K * To)
    x = _Inputs(pred, gt, ns, dev)
    p, g, r = pred.double(), gt.double(), ns.double()[:, 1]
    d = (p[:, 0] - g) * r[:, None, None]                # [B, 2, To], candidate 0
    assert bool((d == d.round()).all()) and d.abs().max().item() <= 12
    want = (d * d).sum((0, 2))
    assert 2 * want.max().item() < 2.0 ** 24
    what = f"traj_metrics integer {(B, K, To)}"
    s1, _, _ = _call(x, dev, what)
    assert s1.region[0, :2].double().cpu().tolist() == want.tolist(), f"{what}: sums[0..1] {s1.region[0, :2].tolist()} != {want.tolist()}"
    s2, _, _ = _call(x, dev, what + " accumulated", start=s1.region.cpu(), outputs=False)
    assert s2.region[0, :2].double().cpu().tolist() == (2 * want).tolist(), f"{what}: accumulated sums[0..1] {s2.region[0, :2].tolist()} != {(2 * want).tolist()}"


@pytest.mark.parametrize("bad", ["nan", "inf"])
@pytest.mark.parametrize("B,K,To", SHAPES)
def test_nonfinite_reaches_the_loss(gpu, B, K, To, bad):
    """one NaN in x / one +inf in y of candidate 0 of one sample: sums[0] / sums[1] is not finite; the other samples' per_sample rows
    come back finite and inside their bounds"""
    dev = gpu["device"]
    pred, gt, ns = _batch(B, K, To, 5000 + B * K * To)
    ref = _reference(pred, gt, ns)
    b0, t0, c = (2 * B) // 3, To // 2, 0 if bad == "nan" else 1
    pred[b0, 0, c, t0] = float(bad)
    x = _Inputs(pred, gt, ns, dev)
    what = f"traj_metrics {bad} {(B, K, To)}"
    sums, _, per = _call(x, dev, what)
    s = sums.region[0].cpu()
    assert not bool(torch.isfinite(s[c])), f"{what}: sums[{c}] = {s[c].item()} is finite"
    assert bool(torch.isfinite(s[1 - c])), f"{what}: sums[{1 - c}] = {s[1 - c].item()}: the other coordinate's sum is not finite"
    if bad == "inf":
        assert s[1].item() == float("inf")
    keep = torch.arange(B) != b0
    if bool(keep.any()):
        for i, k in enumerate(("ade", "fde", "rmse")):
            _judge(per.region[:, i].cpu()[keep], ref[k][keep], ref["d" + k][keep], f"{what} per_sample {k} of the other samples", "per_sample " + k)


def test_refusals(gpu):
    dev = gpu["device"]
    d = torch.zeros(64, device=dev).data_ptr()
    sums, per = _guarded(1, 5, F32, dev, fill=torch.ones(1, 5)), _guarded(2, 3, F32, dev)
    L = _L()
    _refused(L.tcavt_traj_metrics(None, d, d, sums.ptr, None, per.ptr, 2, 1, 4, _st()), "traj_metrics", [sums, per], "pred NULL")
    _refused(L.tcavt_traj_metrics(d, None, d, sums.ptr, None, per.ptr, 2, 1, 4, _st()), "traj_metrics", [sums, per], "gt NULL")
    _refused(L.tcavt_traj_metrics(d, d, None, sums.ptr, None, per.ptr, 2, 1, 4, _st()), "traj_metrics", [sums, per], "norm_stat NULL")
    _refused(L.tcavt_traj_metrics(d, d, d, None, None, per.ptr, 2, 1, 4, _st()), "traj_metrics", [sums, per], "sums NULL")
    _refused(L.tcavt_traj_metrics(d, d, d, sums.ptr, None, per.ptr, 0, 1, 4, _st()), "traj_metrics", [sums, per], "B = 0")
    _refused(L.tcavt_traj_metrics(d, d, d, sums.ptr, None, per.ptr, 2, 0, 4, _st()), "traj_metrics", [sums, per], "K = 0")
    _refused(L.tcavt_traj_metrics(d, d, d, sums.ptr, None, per.ptr, 2, 1, 0, _st()), "traj_metrics", [sums, per], "To = 0")


def test_report_worst_ratio(gpu):
    """(runs last in file order) prints the worst fraction of the bound measured in this session"""
    for k in sorted(_WORST):
        print(f"tcavt_traj_metrics   {k:20s} worst frac {_WORST[k]:7.3f}")
