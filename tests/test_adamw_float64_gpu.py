"""tcavt_adamw and tcavt_adamw_gated (csrc/backward.hip) against float64, called on their own: p, m AND v per element.

Every case calls the C entry point (capi.lib().tcavt_adamw*) and checks every element against ONE float64 evaluation of the update
in torch on the CPU, from the same fp32 values and the hyper-parameters rounded to fp32 as the kernel receives them; nothing in a
reference comes from a project kernel or from torch.optim.  p, m and v lie between NaN guards, g has NaN behind it, ctl sits between
sentinel rows: every guard keeps its bits, g stays bit-unchanged, a second launch from the same state gives the same bits.

| n | why (the grid is min(ceil(n / 256), 8192) blocks of 256 threads, grid-stride loop) |
|---|---|
| 1, 255, 256, 257 | one thread; a ragged block; one whole block; one element in a second block |
| 65 537 | 257 blocks, the last with one element |
| 2 097 152 | 8192 * 256: the largest n with a single loop iteration |
| 4 194 381 = 2 * 2 097 152 + 77 | a whole second iteration and a third with a ragged tail of 77 |

State and hyper-parameters: zero moments at step 1; given m, v at steps 2, 3, 10, 1000 (tcavt_adamw: `step`; gated: ctl[0] preset to
step - 1, ctl[4], ctl[5] checked against 1 - b^t); grad_scale 1, 0.5, 1/3; weight_decay 0, 1e-2; lr = 3e-3, betas (0.9, 0.999),
eps = 1e-8.  All 30 combinations run at n <= 65 537, two each at the two large sizes.

One vector holds three parameter magnitudes (0, ~1e-4, ~1: where |p| is small the check on p is a check on the update) and three
kinds of special gradient entries:
- g == 0 with zero moments: the update is exactly 0, m and v stay 0, p = p * (1 - lr * wd) bit for bit (p only decays);
- |g| = 1e-20: g^2 leaves the normal fp32 range, v comes out subnormal (no flush to zero: the bound allows one subnormal spacing per
  operation), sqrt(vhat) vanishes against eps and the update is lr * mhat / eps -- as the float64 reference says;
- |g| = 1e15: (1 - b2) g^2 ~ 1e27 approaches the top of the range, nothing overflows and the update is ~ lr * sign(g).
That is the kernel's contract at the edges of the range, asserted within the same bounds as everything else.

Exact regime: b1 = b2 = 0.5, step 1, eps = 0, wd = 0, lr = 2^-10, zero moments, g = +-2^j, p a multiple of 2^-12: m = g / 2,
v = g^2 / 2, the update lr * sign(g), all exact -- p, m, v equal the float64 values bit for bit at every n.

Gate semantics and the back-off of tcavt_adamw_gated are tested elsewhere (test_adamw_gated_skips_nonfinite_loss); here the same
matrix runs through it with a finite loss, and one skipped call (NaN loss) at the largest n keeps every bit of p, m, v and the guards.

Refusals pass only arguments that the host code rejects before any launch (NULL pointers, n = 0, step = 0).

MEASURED on an MI355X: the worst fraction of the bound per output stands beside the constants below;
profiles/fp32_train_tail_bounds.txt has every line, the powf probe and the mutants; test_report_worst_ratio prints the session's.
"""
import pytest
import torch

from test_attention_bwd_gpu import _first_bad, _last_error
from test_gemm_forms_gpu import _ulp
from test_llm_backward_kernels_gpu import _gen, _L, _ok, _st

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
_E = 2.0 ** -24        # unit roundoff of fp32
_ETA = 2.0 ** -149     # spacing of the fp32 subnormals: the absolute error of an operation whose result underflows
# powf(b, t) in the bias corrections: host libm in tcavt_adamw, the device library in adamw_gate_kernel.  No accuracy table of the
# device library is installed with the toolchain, so it was measured on an MI355X (a probe of its own, device powf against float64
# pow): over the bases and steps used here (0.9, 0.999, 0.5 at steps 1, 2, 3, 10, 1000) worst 0.508 ulp on the device, 0.492 ulp in
# host libm (over six bases and steps 1..4096: 1.187 and 0.608).  Used with a margin of one ulp: 1.508 ulp, 2 E relative each.
_POW_ULPS = 0.508 + 1.0
_C_POW = 2.0 * _POW_ULPS
# MEASURED on an MI355X: worst fraction of the whole bound (bar 1.0) over all realistic cases
#   tcavt_adamw        p 0.380   m 0.484   v 0.535
#   tcavt_adamw_gated  p 0.380   m 0.484   v 0.535   ctl[4..5] 0.170
# Mutants (profiles/fp32_train_tail_bounds.txt): bias correction of step - 1, eps inside the square root, decay after the update,
# v from the unscaled gradient, the loop reduced to one iteration: each fails here.
_WORST = {}

_BLOCK, _MAX_BLOCKS = 256, 8192
_FULL = _BLOCK * _MAX_BLOCKS                         # 2 097 152 elements per loop iteration of a full grid
SIZES = [1, 255, 256, 257, 65_537, _FULL, 2 * _FULL + 77]
STEPS = [1, 2, 3, 10, 1000]
SCALES = [1.0, 0.5, 1.0 / 3.0]
DECAYS = [0.0, 1e-2]
ALL = [(s, gs, wd) for s in STEPS for gs in SCALES for wd in DECAYS]
LARGE = {_FULL: [(1, 1.0 / 3.0, 1e-2), (1000, 0.5, 0.0)], 2 * _FULL + 77: [(1, 0.5, 0.0), (10, 1.0 / 3.0, 1e-2)]}
ENTRIES = ["tcavt_adamw", "tcavt_adamw_gated"]
LR, B1, B2, EPS = 3e-3, 0.9, 0.999, 1e-8


def _configs(n):
    return LARGE.get(n, ALL)


def _launch(n):
    """(blocks, loop iterations of thread 0, elements in the last iteration) of adamw_kernel / adamw_gated_kernel"""
    blocks = min(-(-n // _BLOCK), _MAX_BLOCKS)
    stride = blocks * _BLOCK
    return blocks, -(-n // stride), (n - 1) % stride + 1


def test_cases_cover_the_host_rules():
    """from the case lists alone (the launch arithmetic of both entry points mirrored): every path and edge is reached"""
    la = {n: _launch(n) for n in SIZES}
    assert la[1] == (1, 1, 1) and la[255] == (1, 1, 255) and la[256] == (1, 1, 256) and la[257] == (2, 1, 257)
    assert la[65_537] == (257, 1, 65_537)
    assert la[_FULL] == (_MAX_BLOCKS, 1, _FULL)                       # the cap is reached, still one iteration
    assert la[2 * _FULL + 77] == (_MAX_BLOCKS, 3, 77)                 # a whole second iteration, a ragged third
    assert max(SIZES) * 4 < 17 * 2 ** 20                              # 4.2 M floats
    for n in SIZES:
        cs = _configs(n)
        assert any(s == 1 for s, _, _ in cs) and any(s > 1 for s, _, _ in cs)
        assert any(gs not in (1.0, 0.5) for _, gs, _ in cs) and {wd for _, _, wd in cs} == set(DECAYS)
    small = [n for n in SIZES if n not in LARGE]
    assert all(set(_configs(n)) == set(ALL) for n in small) and len(ALL) == 30 and max(small) > 256
    assert set(STEPS) == {1, 2, 3, 10, 1000} and 1.0 / 3.0 in SCALES


# ---------------------------------------------------------------------------------------------------------------------------
# data, reference and bound

def _f(x):
    """x rounded to fp32, as a Python float (what a c_float argument holds)"""
    return torch.tensor(x, dtype=F32).item()


def _kinds(n):
    """0: ordinary, 1: g == 0 with zero moments, 2: |g| = 1e-20, 3: |g| = 1e15"""
    i = torch.arange(n) % 97
    return (i == 5) * 1 + (i == 11) * 2 + (i == 17) * 3


def _state(n, step, seed):
    """fp32 tensors on the CPU: p in three magnitudes (0, ~1e-4, ~1), g ~ 1e-2 with the special entries, m, v zero at step 1"""
    g_ = _gen(seed)
    mag = torch.tensor([0.0, 1e-4, 1.0])[torch.arange(n) % 3]
    p = torch.randn(n, generator=g_) * mag
    g = torch.randn(n, generator=g_) * 1e-2
    sign = torch.where(torch.rand(n, generator=g_) < 0.5, -1.0, 1.0)
    kind = _kinds(n)
    g = torch.where(kind == 1, torch.zeros(n), g)
    g = torch.where(kind == 2, 1e-20 * sign, g)
    g = torch.where(kind == 3, 1e15 * sign, g)
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m, v = torch.randn(n, generator=g_) * 1e-2, (torch.randn(n, generator=g_) * 1e-2) ** 2
        m, v = torch.where(kind == 1, torch.zeros(n), m), torch.where(kind == 1, torch.zeros(n), v)
    return p, g, m, v, kind


def _reference(p, g, m, v, step, gs, wd, lr=LR, b1=B1, b2=B2, eps=EPS):
    """float64 p', m', v' and their fp32 bounds, from the chain of adamw_kernel (-ffp-contract=off: every operation rounds once,
    E = 2^-24; an operation whose result underflows errs by at most ETA = 2^-149 instead):
      gi = g * gs                                                           one rounding
      mi = b1 * m + (1 - b1) * gi:  A = b1 m rounds once, B = (1 - b1) gi carries 1 - b1, gi and the product (3 E), the sum E (|A| + |B|)
                                    dm = E (2 |A| + 4 |B|) + 3 ETA
      vi = b2 * v + (1 - b2) * gi * gi:  B carries 1 - b2, gi twice and two products (5 E)
                                    dv = E (2 |A| + 6 |B|) + 4 ETA
      bc = 1 - powf(b, step):       dbc = C_POW E b^t + ETA + E bc          -- relative to bc it is amplified by b^t / (1 - b^t),
                                                                               ~1000 for b2 at step 1; carried as its own term
      mh = mi / bc1, vh = vi / bc2, D = sqrtf(vh) + eps:
                                    dD = sqrt(vh) (dv / (2 v') + (dbc2 / bc2 + E) / 2 + E) + E D
      upd = lr * mh / D:            dupd = lr dm / (bc1 D) + |upd| (dbc1 / bc1 + 3 E + dD / D) + ETA
      p' = p * (1 - lr * wd) - upd: dp = 3 E |p (1 - lr wd)| + E |p'| + dupd + ETA
    (sqrtf and the divisions round correctly: one E each.)"""
    lr, b1, b2, eps, wd, gs = (_f(x) for x in (lr, b1, b2, eps, wd, gs))
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gi = g * gs
    A, Bm = b1 * m, (1 - b1) * gi
    m2, dm = A + Bm, _E * (2 * A.abs() + 4 * Bm.abs()) + 3 * _ETA
    Av, Bv = b2 * v, (1 - b2) * gi * gi
    v2, dv = Av + Bv, _E * (2 * Av + 6 * Bv) + 4 * _ETA
    bc, dbc = [], []
    for b in (b1, b2):
        pw = b ** step
        bc.append(1 - pw)
        dbc.append(_C_POW * _E * pw + _ETA + _E * (1 - pw))
    mh, vh = m2 / bc[0], v2 / bc[1]
    s = vh.sqrt()
    D = s + eps
    dD = s * (torch.where(v2 > 0, dv / (2 * v2).clamp_min(1e-300), torch.zeros_like(v2)) + (dbc[1] / bc[1] + _E) / 2 + _E) + _E * D
    upd = lr * mh / D
    dupd = lr * dm / (bc[0] * D) + upd.abs() * (dbc[0] / bc[0] + 3 * _E + dD / D) + _ETA
    p0 = p * (1 - lr * wd)
    p2 = p0 - upd
    dp = 3 * _E * p0.abs() + _E * p2.abs() + dupd + _ETA
    return {"p": (p2, dp), "m": (m2, dm), "v": (v2, dv), "bc": (bc, dbc), "upd": upd}


class _Vec:
    """n fp32 values between two 64-element NaN guards"""
    G = 64

    def __init__(self, t, dev):
        self.n = t.numel()
        self.buf = torch.full((self.n + 2 * self.G,), float("nan"), dtype=F32, device=dev)
        self.region.copy_(t)
        self.before = self.buf.clone()

    @property
    def region(self):
        return self.buf[self.G: self.G + self.n]

    @property
    def ptr(self):
        return self.region.data_ptr()

    def guards_kept(self, what):
        for sl in (slice(0, self.G), slice(self.G + self.n, None)):
            assert torch.equal(self.buf[sl].view(torch.int32), self.before[sl].view(torch.int32)), f"{what}: write outside the {self.n} elements"

    def unchanged(self, what):
        assert torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32)), f"{what}: modified"


class _Ctl:
    """ctl int32[8] between two sentinel rows"""

    def __init__(self, applied, dev):
        self.buf = torch.full((3, 8), -777, dtype=torch.int32, device=dev)
        self.buf[1] = torch.tensor([applied, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32)
        self.before = self.buf.clone()

    @property
    def ptr(self):
        return self.buf[1].data_ptr()

    def guards_kept(self, what):
        assert torch.equal(self.buf[0::2], self.before[0::2]), f"{what}: write outside ctl[8]"


def _run(entry, dev, p, g, m, v, step, gs, wd, what, lr=LR, b1=B1, b2=B2, eps=EPS, loss=1.0):
    """two launches from the same state into fresh guarded buffers: status, guards, g unchanged, reproducibility.
    Returns the (p, m, v, ctl) buffers of the first"""
    runs = []
    gv = _Vec(g, dev)
    for tag in ("", " again"):
        pv, mv, vv = _Vec(p, dev), _Vec(m, dev), _Vec(v, dev)
        ctl = None
        if entry == "tcavt_adamw":
            rc = _L().tcavt_adamw(pv.ptr, gv.ptr, mv.ptr, vv.ptr, p.numel(), lr, b1, b2, eps, wd, step, gs, _st())
        else:
            ctl = _Ctl(step - 1, dev)
            lo = torch.tensor([float("nan"), loss, float("nan")], dtype=F32, device=dev)
            rc = _L().tcavt_adamw_gated(pv.ptr, gv.ptr, mv.ptr, vv.ptr, p.numel(), lr, b1, b2, eps, wd, gs, lo[1:].data_ptr(), None, ctl.ptr, _st())
        _ok(rc, what + tag)
        for o in (pv, mv, vv) + ((ctl,) if ctl else ()):
            o.guards_kept(what + tag)
        gv.unchanged(what + tag + ": g")
        runs.append((pv, mv, vv, ctl))
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert torch.equal(a.region.view(torch.int32), b.region.view(torch.int32)), what + ": not reproducible"
    if runs[0][3] is not None:
        assert torch.equal(runs[0][3].buf, runs[1][3].buf), what + ": ctl not reproducible"
    return runs[0]


def _judge(got, ref, f32, what, key):
    """|got - ref| <= 1.01 * f32 + ulp_fp32(ref) per element, every element finite; records the worst fraction"""
    g = got.double().cpu()
    assert torch.isfinite(g).all(), f"{what}: {int((~torch.isfinite(g)).sum())} non-finite elements"
    bound = 1.01 * f32 + _ulp(ref, F32)
    d = (g - ref).abs()
    frac = (d / bound).max().item()
    _WORST[key] = max(_WORST.get(key, -1.0), frac)
    bad = d > bound
    if bool(bad.any()):
        i = _first_bad(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of bound (worst fraction {frac:.3f}); first {i}: "
                             f"got {g[i].item()!r} ref {ref[i].item()!r} allowed {bound[i].item():.3e}")
    return frac


def _check_ctl(ctl, step, ref, what, entry):
    c = ctl.buf[1].cpu()
    assert c[[0, 1, 2, 3, 6, 7]].tolist() == [step, 0, 0, 0, 0, 0], f"{what}: ctl = {c.tolist()}"
    bc, dbc = ref["bc"]
    _judge(c[4:6].view(F32), torch.tensor(bc, dtype=F64), torch.tensor(dbc, dtype=F64), what + " ctl[4..5]", (entry, "ctl[4..5]"))


# ---------------------------------------------------------------------------------------------------------------------------
# tests

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_against_float64(gpu, entry, n):
    dev = gpu["device"]
    for ci, (step, gs, wd) in enumerate(_configs(n)):
        p, g, m, v, kind = _state(n, step, 7000 + 31 * ci + n % 1000)
        what = f"{entry} n={n} step={step} grad_scale={gs:.3g} wd={wd}"
        ref = _reference(p, g, m, v, step, gs, wd)
        pv, mv, vv, ctl = _run(entry, dev, p, g, m, v, step, gs, wd, what)
        fr = [_judge(o.region, ref[k][0], ref[k][1], f"{what} {k}", (entry, k)) for o, k in ((pv, "p"), (mv, "m"), (vv, "v"))]
        if n in LARGE:
            print(f"frac {what}: p {fr[0]:.3f} m {fr[1]:.3f} v {fr[2]:.3f}")
        if ctl is not None:
            _check_ctl(ctl, step, ref, what, entry)
        # g == 0 with zero moments: no update at all, p only decays
        z = kind == 1
        if bool(z.any()):
            c32 = torch.tensor(1.0, dtype=F32) - torch.tensor(LR, dtype=F32) * torch.tensor(wd, dtype=F32)
            assert bool((ref["upd"][z] == 0).all())
            assert torch.equal((p[z] * c32).view(torch.int32), pv.region.cpu()[z].view(torch.int32)), what + ": p moved where g, m and v are 0"
            assert bool((mv.region.cpu()[z] == 0).all()) and bool((vv.region.cpu()[z] == 0).all()), what + ": moments of a zero gradient"
        # the edges of the range, as the reference has them: v subnormal but not 0 / everything finite
        if step == 1 and bool((kind == 2).any()):
            sub = vv.region.cpu()[kind == 2]
            assert bool((sub > 0).all()) and bool((sub < 2.0 ** -126).all()), what + ": v of |g| = 1e-20 is not a subnormal"
        if step == 1 and bool((kind == 3).any()):
            big = ref["upd"][kind == 3].abs()
            assert bool((big > 0.99 * LR).all()) and bool((big < 1.01 * LR).all())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_exact_regime(gpu, entry, n):
    """b1 = b2 = 0.5, step 1, eps = 0, wd = 0, lr = 2^-10, zero moments, g = +-2^j: m = g / 2, v = g^2 / 2, p - lr sign(g), bit for bit"""
    dev = gpu["device"]
    g_ = _gen(8000 + n % 1000)
    lr = 2.0 ** -10
    p = torch.randint(-4 * 4096, 4 * 4096 + 1, (n,), generator=g_).float() / 4096
    sign = torch.where(torch.rand(n, generator=g_) < 0.5, -1.0, 1.0)
    g = sign * torch.ldexp(torch.ones(n), torch.randint(-10, 11, (n,), generator=g_))
    z = torch.zeros(n)
    what = f"{entry} exact n={n}"
    pv, mv, vv, ctl = _run(entry, dev, p, g, z, z, 1, 1.0, 0.0, what, lr=lr, b1=0.5, b2=0.5, eps=0.0)
    g64 = g.double()
    want = {"p": p.double() - lr * g64.sign(), "m": g64 / 2, "v": g64 * g64 / 2}
    for o, k in ((pv, "p"), (mv, "m"), (vv, "v")):
        assert bool((want[k].float().double() == want[k]).all())
        bad = o.region.cpu().view(torch.int32) != want[k].float().view(torch.int32)
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements of {k} differ in bits; first {_first_bad(bad)}"
    if ctl is not None:
        c = ctl.buf[1].cpu()
        assert c[0].item() == 1 and c[4:6].view(F32).tolist() == [0.5, 0.5], f"{what}: ctl = {c.tolist()}"


def test_gated_skip_keeps_every_bit(gpu):
    """one skipped call (NaN loss) at the largest n: p, m, v and the guards keep their bits"""
    dev = gpu["device"]
    n = SIZES[-1]
    p, g, m, v, _ = _state(n, 10, 9000)
    pv, mv, vv, gv, ctl = _Vec(p, dev), _Vec(m, dev), _Vec(v, dev), _Vec(g, dev), _Ctl(9, dev)
    lo = torch.tensor([1.0, float("nan"), 1.0], dtype=F32, device=dev)
    _ok(_L().tcavt_adamw_gated(pv.ptr, gv.ptr, mv.ptr, vv.ptr, n, LR, B1, B2, EPS, 1e-2, 1.0, lo[1:].data_ptr(), None, ctl.ptr, _st()), "skipped call")
    for o, k in ((pv, "p"), (mv, "m"), (vv, "v"), (gv, "g")):
        o.unchanged(f"tcavt_adamw_gated skipped n={n}: {k}")
    ctl.guards_kept("skipped call")
    assert ctl.buf[1, :3].tolist() == [9, 1, 1]


def test_refusals(gpu):
    dev = gpu["device"]
    vec = [_Vec(torch.ones(8), dev) for _ in range(4)]
    p, g, m, v = (x.ptr for x in vec)
    ctl, lo = _Ctl(0, dev), torch.ones(1, device=dev)
    L = _L()

    def refused(rc, name, what):
        torch.cuda.synchronize()
        assert rc != 0, f"{what}: accepted"
        assert _last_error().startswith(name + ":"), f"{what}: tcavt_last_error() = {_last_error()!r} does not name {name}"
        for x in vec:
            x.unchanged(what)
        assert torch.equal(ctl.buf, ctl.before), f"{what}: ctl written"

    hp = (LR, B1, B2, EPS, 1e-2)
    for i, nm in enumerate("pgmv"):
        a = [p, g, m, v]
        a[i] = None
        refused(L.tcavt_adamw(*a, 8, *hp, 1, 1.0, _st()), "adamw", f"adamw {nm} NULL")
        refused(L.tcavt_adamw_gated(*a, 8, *hp, 1.0, lo.data_ptr(), None, ctl.ptr, _st()), "adamw_gated", f"adamw_gated {nm} NULL")
    refused(L.tcavt_adamw(p, g, m, v, 0, *hp, 1, 1.0, _st()), "adamw", "adamw n = 0")
    refused(L.tcavt_adamw(p, g, m, v, 8, *hp, 0, 1.0, _st()), "adamw", "adamw step = 0")
    refused(L.tcavt_adamw_gated(p, g, m, v, 0, *hp, 1.0, lo.data_ptr(), None, ctl.ptr, _st()), "adamw_gated", "adamw_gated n = 0")
    refused(L.tcavt_adamw_gated(p, g, m, v, 8, *hp, 1.0, None, None, ctl.ptr, _st()), "adamw_gated", "adamw_gated loss NULL")
    refused(L.tcavt_adamw_gated(p, g, m, v, 8, *hp, 1.0, lo.data_ptr(), None, None, _st()), "adamw_gated", "adamw_gated ctl NULL")


def test_report_worst_ratio(gpu):
    """(runs last in file order) prints the worst fraction of the bound measured in this session per entry and output"""
    for k in sorted(_WORST):
        print(f"{k[0]:18s} {k[1]:10s} worst frac {_WORST[k]:7.3f}")
