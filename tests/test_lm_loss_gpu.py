"""tcavt_lm_loss_forward / tcavt_lm_loss_backward through the C entry points against float64, in fp16 and bf16.

The reference is evaluated on the GPU in float64 from the SAME 16-bit operands, in row blocks: z = h W^T, lse, the per-row
loss, the mean, and G = (g / N) (softmax(z) - onehot) W.  Outputs (loss, count, lse, row_loss, g_out) live inside larger
NaN-filled buffers; h16 has NaN padding columns and NaN rows, the table and its transpose NaN rows / columns after the
part the contract names; h16, table, table_t, labels, kv_len and g_loss must be bit-unchanged after the calls.

Bounds (U = 2^-24, A = |h| |W|^T in float64):
  lse, row loss : _C_ACC * U * A[row, argmax z] + 4 ulp_fp32(lse)
  mean loss     : 1e-6 relative
  count         : exact
  g_out element : 1/2 ulp_out(ref) + (g / N) * sum_v (u_P(p_v) + _C_BWD * U * |p_v| * A_v) * |W_vj|
                  u_P = half an ulp of P's 16-bit type at |p_v|; fp16 holds 2^14 P, so its subnormal spacing is 2^-38 in P
  unlabelled rows of g_out: bit zero; of lse / row_loss: zero
Every labelled row and every output element is compared.  test_report_worst_ratio prints the worst measured c (pytest -s).
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
U = 2.0 ** -24
# forward accumulator bar (the project's form, tests/test_gemm_forms_gpu.py).  Measured on an MI355X: worst c = 1.82 (one
# logit 60 above the others, fp16; 0.46 at V 128256 x H 2048 with random operands)
_C_ACC = 4.0
# backward bar: at most 4 x the worst measured ratio.  Measured on an MI355X: 0 in every case -- no element leaves
# 1/2 ulp_out + (g / N) sum_v u_P(p_v) |W_vj|, the rounding of P alone (a worst-case sum: all roundings aligned), so the
# accumulator term gets no allowance at all.  The largest fraction of that bound any element uses is printed (0.99 measured,
# where P is all but one-hot and what is left is the output's own rounding)
_C_BWD = 0.0
_WORST = {}
MIB = 1 << 20
CAP = 640 * MIB


def _capi():
    from tcavt_amd import capi

    return capi


def _bits(t):
    return t.view({F32: torch.int32, F16: torch.int16, BF16: torch.int16, torch.int32: torch.int32, torch.int64: torch.int64}[t.dtype])


def _ulp(x, dt, emin=None):
    """ulp of dt at |x| (float64 tensor), subnormal spacing below the normal range"""
    p, e0 = {F16: (10, -14), BF16: (7, -126), F32: (23, -126)}[dt]
    emin = e0 if emin is None else emin
    _, e = torch.frexp(x)
    e = torch.where(x == 0, torch.full_like(e, emin + 1), e)
    return torch.ldexp(torch.ones_like(x), (e - 1).clamp_min(emin) - p)


def _u_p(p, dt):
    """rounding unit of the kernel's 16-bit P at |p|: fp16 operands hold 2^14 P (normal down to 2^-28, spacing 2^-38 below)"""
    return 0.5 * _ulp(p, dt, emin=-28 if dt == F16 else None)


class Poisoned:
    """A [rows, cols] region inside a NaN-filled [rows + extra_rows, ld] buffer."""

    def __init__(self, rows, cols, dt, dev, ld=None, extra_rows=2, fill=None):
        self.ld = cols + 16 if ld is None else ld
        self.buf = torch.full((rows + extra_rows, self.ld), float("nan"), dtype=dt, device=dev)
        self.rows, self.cols = rows, cols
        if fill is not None:
            self.buf[:rows, :cols] = fill.to(dt)
        self.before = self.buf.clone()

    @property
    def region(self):
        return self.buf[: self.rows, : self.cols]

    def check_outside(self, what):
        out = torch.ones_like(self.buf, dtype=torch.bool)
        out[: self.rows, : self.cols] = False
        assert torch.equal(_bits(self.buf)[out], _bits(self.before)[out]), f"{what}: write outside [{self.rows}, {self.cols}]"

    def check_unchanged(self, what):
        assert torch.equal(_bits(self.buf), _bits(self.before)), f"{what}: input changed"


def expected_targets(labels, B, L, Nq, V, kv_len=None):
    """Row -> target (or -1) as the issue states the semantics, plus whether a bad label was met (a host loop on purpose)."""
    lab = labels.cpu().tolist()
    kv = None if kv_len is None else kv_len.cpu().tolist()
    tgt, bad = [-1] * (B * L), False
    for b in range(B):
        for p in range(L - 1):
            t = -100 if p + 1 < Nq else lab[b][p + 1 - Nq]
            if t == -100:
                continue
            if t < 0 or t >= V or (kv is not None and p + 1 >= kv[b]):
                bad = True
                continue
            tgt[b * L + p] = t
    return torch.tensor(tgt, dtype=torch.int64), bad


class LmRun:
    """One forward (+ backward) call on operands given in float64 (rounded to `dt` here)."""

    def __init__(self, h, W, labels, B, L, Nq, dt, kv_len=None, g_loss=None, gdt=BF16, backward=True, ws_bytes=None):
        capi = _capi()
        dev = torch.device("cuda")
        self.B, self.L, self.Nq, self.dt, self.gdt = B, L, Nq, dt, gdt
        R, (V, H) = B * L, W.shape
        self.R, self.V, self.H = R, V, H
        Vp = (V + 63) // 64 * 64
        self.pH = Poisoned(R, H, dt, dev, ld=H + 64, extra_rows=3, fill=h)
        self.pW = Poisoned(V, H, dt, dev, ld=H, extra_rows=3, fill=W)
        wt = torch.zeros(H, Vp, dtype=dt, device=dev)
        wt[:, :V] = self.pW.region.t()
        self.pWT = Poisoned(H, Vp, dt, dev, ld=Vp + 64, extra_rows=2, fill=wt)
        del wt
        self.labels = labels.to(dev).contiguous()
        self.labels0 = self.labels.clone()
        self.kv_len = None if kv_len is None else kv_len.to(dev).to(torch.int32).contiguous()
        self.kv0 = None if kv_len is None else self.kv_len.clone()
        self.g_loss = None if g_loss is None else torch.tensor([g_loss], dtype=F32, device=dev)
        nan = float("nan")
        self.loss = torch.full((4,), nan, dtype=F32, device=dev)
        self.count = torch.full((4,), -12345, dtype=torch.int32, device=dev)
        self.flag = torch.zeros(4, dtype=torch.int32, device=dev)
        self.lse = torch.full((R + 8,), nan, dtype=F32, device=dev)
        self.row_loss = torch.full((R + 8,), nan, dtype=F32, device=dev)
        self.pG = Poisoned(R, H, gdt, dev, ld=H + 16)
        need = capi.lib().tcavt_lm_loss_workspace_bytes(R, V, H)
        self.ws_need = need
        self.ws = torch.full((need if ws_bytes is None else ws_bytes,), 0xFF, dtype=torch.uint8, device=dev)
        a = capi.LmLossArgs()
        a.h16, a.ldh, a.table = self.pH.buf.data_ptr(), self.pH.ld, self.pW.buf.data_ptr()
        a.table_t, a.ldt = self.pWT.buf.data_ptr(), self.pWT.ld
        a.labels = self.labels.data_ptr()
        a.kv_len = None if self.kv_len is None else self.kv_len.data_ptr()
        a.B, a.L, a.V, a.H, a.Nq = B, L, V, H, Nq
        a.dtype16 = capi.F16 if dt == F16 else capi.BF16
        a.grad_dtype = capi.F16 if gdt == F16 else capi.BF16
        a.loss, a.count, a.lse = self.loss[1:].data_ptr(), self.count[1:].data_ptr(), self.lse[4:].data_ptr()
        a.row_loss, a.flag = self.row_loss[4:].data_ptr(), self.flag[1:].data_ptr()
        a.g_loss = None if self.g_loss is None else self.g_loss.data_ptr()
        a.g_out, a.ldg = self.pG.buf.data_ptr(), self.pG.ld
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), self.ws.numel()
        self.args = a
        self.rc_f = capi.lib().tcavt_lm_loss_forward(ctypes.byref(a), capi.stream_ptr())
        self.rc_b = capi.lib().tcavt_lm_loss_backward(ctypes.byref(a), capi.stream_ptr()) if backward and self.rc_f == 0 else None
        torch.cuda.synchronize()

    def rerun(self):
        capi = _capi()
        assert capi.lib().tcavt_lm_loss_forward(ctypes.byref(self.args), capi.stream_ptr()) == 0
        assert capi.lib().tcavt_lm_loss_backward(ctypes.byref(self.args), capi.stream_ptr()) == 0
        torch.cuda.synchronize()

    def check_buffers(self, what, backward=True):
        for p, n in ((self.pH, "h16"), (self.pW, "table"), (self.pWT, "table_t")):
            p.check_unchanged(f"{what}: {n}")
        assert torch.equal(self.labels, self.labels0), f"{what}: labels changed"
        if self.kv_len is not None:
            assert torch.equal(self.kv_len, self.kv0)
        assert torch.isnan(self.loss[0]) and torch.isnan(self.loss[2:]).all(), f"{what}: write around loss"
        assert self.count[0] == -12345 and (self.count[2:] == -12345).all(), f"{what}: write around count"
        assert self.flag[0] == 0 and (self.flag[2:] == 0).all(), f"{what}: write around flag"
        for t, n in ((self.lse, "lse"), (self.row_loss, "row_loss")):
            assert torch.isnan(t[:4]).all() and torch.isnan(t[4 + self.R:]).all(), f"{what}: write around {n}"
            assert torch.isfinite(t[4:4 + self.R]).all(), f"{what}: {n} not finite"
        if backward:
            self.pG.check_outside(f"{what}: g_out")

    # outputs
    @property
    def out_loss(self):
        return self.loss[1]

    @property
    def out_count(self):
        return int(self.count[1])

    @property
    def out_flag(self):
        return int(self.flag[1])

    @property
    def out_lse(self):
        return self.lse[4:4 + self.R]

    @property
    def out_row_loss(self):
        return self.row_loss[4:4 + self.R]

    @property
    def out_g(self):
        return self.pG.region


def check_against_f64(run, what, c_bwd=None, key=None):
    """Everything the module docstring bounds, every labelled row and every element of g_out."""
    c_bwd = _C_BWD if c_bwd is None else c_bwd
    dev = run.pH.buf.device
    assert run.rc_f == 0 and run.rc_b == 0, _capi().lib().tcavt_last_error()
    run.check_buffers(what)
    tgt, bad = expected_targets(run.labels, run.B, run.L, run.Nq, run.V, run.kv_len)
    tgt = tgt.to(dev)
    rows = torch.nonzero(tgt >= 0).flatten()
    N = rows.numel()
    assert run.out_count == N, f"{what}: count {run.out_count} != {N}"
    assert run.out_flag == int(bad), f"{what}: flag"
    unl = tgt < 0
    assert torch.equal(_bits(run.out_g)[unl], torch.zeros_like(_bits(run.out_g)[unl])), f"{what}: unlabelled gradient rows not bit zero"
    assert (run.out_lse[unl] == 0).all() and (run.out_row_loss[unl] == 0).all(), f"{what}: unlabelled lse / row loss not zero"
    if N == 0:
        assert torch.isnan(run.out_loss), f"{what}: N = 0 must give a NaN loss"
        return
    W = run.pW.region.double()
    Wabs = W.abs()
    g = 1.0 if run.g_loss is None else float(run.g_loss)
    tot = torch.zeros((), dtype=torch.float64, device=dev)
    worst_f = worst_b = used = 0.0
    blk = max(16, min(256, (1 << 25) // run.V))
    for i in range(0, N, blk):
        r = rows[i:i + blk]
        t = tgt[r]
        h = run.pH.region[r].double()
        z = h @ W.T
        A = h.abs() @ Wabs.T
        lse = torch.logsumexp(z, dim=1)
        zt = z.gather(1, t[:, None])[:, 0]
        rl = lse - zt
        tot += rl.sum()
        amax = A.gather(1, z.argmax(dim=1, keepdim=True))[:, 0]
        acc = U * amax
        ulps = 4 * _ulp(lse, F32)
        for got, ref, nm in ((run.out_lse[r].double(), lse, "lse"), (run.out_row_loss[r].double(), rl, "row loss")):
            err = (got - ref).abs()
            worst_f = max(worst_f, float(((err - ulps).clamp_min(0) / acc.clamp_min(1e-300)).max()) if float(acc.max()) > 0 else 0.0)
            assert (err <= _C_ACC * acc + ulps).all(), f"{what}: {nm} off by {float((err - _C_ACC * acc - ulps).max()):.3e} beyond the bound"
        P = torch.exp(z - lse[:, None])
        P.scatter_add_(1, t[:, None], -torch.ones_like(P[:, :1]))
        ref = (g / N) * (P @ W)
        Pa = P.abs()
        e_round = (g / N) * (_u_p(Pa, run.dt) @ Wabs)
        e_acc = (g / N) * U * ((Pa * A) @ Wabs)
        half = 0.5 * _ulp(ref.abs(), run.gdt)
        err = (run.out_g[r].double() - ref).abs()
        over = (err - half - e_round).clamp_min(0)
        used = max(used, float((err / (half + e_round)).max()))
        if float(e_acc.max()) > 0:
            worst_b = max(worst_b, float((over / e_acc.clamp_min(1e-300))[e_acc > 0].max()))
        bound = half + e_round + c_bwd * e_acc
        assert (err <= bound).all(), f"{what}: g_out off by {float((err - bound).max()):.3e} beyond the bound ({int((err > bound).sum())} elements)"
        del z, A, P, Pa, ref, e_round, e_acc, err, bound
    mean = float(tot) / N
    got = float(run.out_loss)
    assert abs(got - mean) <= 1e-6 * abs(mean), f"{what}: mean loss {got!r} vs {mean!r}"
    k = key or what
    _WORST[k] = (max(_WORST.get(k, (0, 0))[0], worst_f), max(_WORST.get(k, (0, 0))[1], worst_b))
    print(f"[lm_loss] {what}: N = {N}, loss = {got:.6f} (f64 {mean:.6f}), worst c forward = {worst_f:.3f}, backward = {worst_b:.3f} "
          f"(largest fraction of the P-rounding bound used: {used:.3f})")


def _labels(B, Lt, V, g, frac=0.6):
    lab = torch.randint(0, V, (B, Lt), generator=g)
    lab[torch.rand(B, Lt, generator=g) > frac] = -100
    return lab


def _random_case(B, L, Nq, V, H, dt, seed, frac=0.6, scale=1.0, **kw):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(B * L, H, generator=g).double()
    W = (torch.randn(V, H, generator=g) * (scale / math.sqrt(H))).double()
    return LmRun(h, W, _labels(B, L - Nq, V, g, frac), B, L, Nq, dt, **kw)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", [(3, 100, 16, 528, 256), (4, 256, 16, 1024, 512)], ids=["300x528x256", "1024x1024x512"])
def test_forward_backward_against_float64(dt, shape):
    B, L, Nq, V, H = shape
    run = _random_case(B, L, Nq, V, H, dt, seed=V + H, scale=4.0)
    check_against_f64(run, f"{B * L}x{V}x{H} {dt}", key=f"{V}x{H} {dt}")


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_real_vocabulary_against_float64(dt):
    """V = 128256 = 501 x 256 (1002 column tiles, 8 chunks, the last one short), H = 2048, B 4, L 256."""
    run = _random_case(4, 256, 16, 128256, 2048, dt, seed=7, scale=4.0)
    check_against_f64(run, f"1024x128256x2048 {dt}", key=f"128256x2048 {dt}")


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_known_answer_zero_hidden(dt):
    """h = 0: every logit is 0, loss = ln V, gradient row = colsum(W) / V - W[t] (scaled by 1 / N)."""
    B, L, Nq, V, H = 2, 40, 8, 528, 256
    g = torch.Generator().manual_seed(3)
    W = torch.randn(V, H, generator=g).double()
    run = LmRun(torch.zeros(B * L, H, dtype=torch.float64), W, _labels(B, L - Nq, V, g), B, L, Nq, dt)
    check_against_f64(run, f"h = 0 {dt}")
    assert abs(float(run.out_loss) - math.log(V)) <= 1e-6 * math.log(V)
    tgt, _ = expected_targets(run.labels, B, L, Nq, V)
    rows = torch.nonzero(tgt >= 0).flatten().cuda()
    W16 = run.pW.region.double()
    ref = (W16.sum(0)[None, :] / V - W16[tgt[rows.cpu()].cuda()]) / rows.numel()
    # P's rounding only (the accumulator term of the bound is zero here): 1/2 ulp_out + (1 / N) sum_v u_P(p_v) |W_vj|
    p = torch.full((V,), 1.0 / V, dtype=torch.float64, device="cuda")
    e = (_u_p(p, dt)[None, :] @ W16.abs())[0] + _u_p(torch.tensor([1 - 1.0 / V], dtype=torch.float64, device="cuda"), dt) * W16.abs().max(0).values
    err = (run.out_g[rows].double() - ref).abs()
    assert (err <= 0.5 * _ulp(ref.abs(), BF16) + e[None, :] / rows.numel() * 1.01 + 1e-12).all()


def _structured(B, L, V, H, wcol0, wcol1=None, h0=1.0, h1=0.0, noise=0.0, seed=0):
    """h = (h0, h1, noise ...), W[v] = (wcol0[v], wcol1[v], noise ...): z_v = h0 wcol0[v] + h1 wcol1[v] (+ noise)"""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(B * L, H, generator=g).double() * noise
    W = torch.randn(V, H, generator=g).double() * noise
    h[:, 0], h[:, 1] = h0, h1
    W[:, 0] = wcol0
    W[:, 1] = 0.0 if wcol1 is None else wcol1
    return h, W


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("adv", ["ragged_tile", "increasing", "spike60", "equal_large"])
def test_merge_adversaries(dt, adv):
    """Branches of the tile merge that random data never takes (V = 528: four full 128-column tiles and a 16-column one)."""
    B, L, Nq, V, H = 2, 72, 8, 528, 256
    g = torch.Generator().manual_seed(11)
    lab = _labels(B, L - Nq, V, g, frac=0.8)
    v = torch.arange(V, dtype=torch.float64)
    if adv == "ragged_tile":  # target and maximum both in the ragged last tile (columns 512 .. 527)
        col = torch.zeros(V, dtype=torch.float64)
        col[520] = 12.0
        h, W = _structured(B, L, V, H, col, noise=0.125)
        lab[lab >= 0] = 520
        lab[0, 3], lab[1, 5] = 527, 512
    elif adv == "increasing":  # z_v = v / 16 exactly: every tile raises the running maximum
        h, W = _structured(B, L, V, H, torch.floor(v / 16), (v % 16) / 16, h0=1.0, h1=1.0)
    elif adv == "spike60":  # one logit 60 above all others: the others' probabilities are ~ 1e-26
        col = torch.zeros(V, dtype=torch.float64)
        col[300] = 60.0
        h, W = _structured(B, L, V, H, col, noise=0.0625)
        lab[0, :8] = 300
    else:  # all logits equal and large: 128 * 234 = 29952
        h, W = _structured(B, L, V, H, torch.full((V,), 234.0, dtype=torch.float64), h0=128.0)
    run = LmRun(h, W, lab, B, L, Nq, dt)
    check_against_f64(run, f"{adv} {dt}", key=f"adversary {adv} {dt}")
    if adv == "equal_large":
        assert abs(float(run.out_loss) - math.log(V)) <= 4 * 2.0 ** -9  # (fp32 ulp of lse ~ 29958 is 2^-9)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_semantics_shift_ignore_index_and_last_position(dt):
    B, L, Nq, V, H = 3, 40, 16, 528, 256
    g = torch.Generator().manual_seed(5)
    lab = _labels(B, L - Nq, V, g, frac=0.5)
    lab[:, 0] = torch.tensor([17, -100, 400])  # the last image row (p = Nq - 1) predicts labels[:, 0]
    lab[:, -1] = torch.tensor([3, 4, -100])
    h = torch.randn(B * L, H, generator=g).double()
    W = (torch.randn(V, H, generator=g) / 4).double()
    run = LmRun(h, W, lab, B, L, Nq, dt)
    check_against_f64(run, f"semantics {dt}")
    lse = run.out_lse.view(B, L)
    assert lse[0, Nq - 1] != 0 and lse[1, Nq - 1] == 0 and lse[2, Nq - 1] != 0  # image/text boundary
    assert (lse[:, : Nq - 1] == 0).all()      # image rows before it predict image tokens: never labelled
    assert (lse[:, L - 1] == 0).all()         # the last position predicts nothing
    assert lse[0, L - 2] != 0 and lse[2, L - 2] == 0  # row L - 2 predicts labels[:, -1]
    assert run.out_count == int((lab != -100).sum())


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_no_labelled_row(dt):
    """N = 0: NaN loss (0 / 0, as torch), all-zero gradient, no fault."""
    B, L, Nq, V, H = 2, 40, 8, 528, 256
    g = torch.Generator().manual_seed(6)
    h = torch.randn(B * L, H, generator=g).double()
    W = torch.randn(V, H, generator=g).double()
    run = LmRun(h, W, torch.full((B, L - Nq), -100, dtype=torch.int64), B, L, Nq, dt)
    check_against_f64(run, f"N = 0 {dt}")
    assert run.out_count == 0 and torch.isnan(run.out_loss)
    assert torch.equal(_bits(run.out_g), torch.zeros_like(_bits(run.out_g)))


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_bad_labels_set_the_flag_and_drop_the_row(dt):
    B, L, Nq, V, H = 2, 40, 8, 528, 256
    g = torch.Generator().manual_seed(8)
    h = torch.randn(B * L, H, generator=g).double()
    W = (torch.randn(V, H, generator=g) / 4).double()
    lab = _labels(B, L - Nq, V, g, frac=0.7)
    kv = torch.tensor([L, L - 6])
    lab[1, L - Nq - 6:] = -100  # sample 1's padding carries no labels in the clean case
    clean = LmRun(h, W, lab, B, L, Nq, dt, kv_len=kv)
    check_against_f64(clean, f"clean {dt}")
    assert clean.out_flag == 0
    for what, (b, j, val) in {"label == V": (0, 4, V), "negative label": (0, 9, -5), "label beyond kv_len": (1, L - Nq - 3, 7)}.items():
        bad = lab.clone()
        was = int(bad[b, j])
        bad[b, j] = val
        run = LmRun(h, W, bad, B, L, Nq, dt, kv_len=kv)
        check_against_f64(run, f"{what} {dt}")  # (expected_targets excludes the row and expects the flag)
        assert run.out_flag == 1, what
        assert run.out_count == clean.out_count - (was != -100)
        ref = lab.clone()
        ref[b, j] = -100
        same = LmRun(h, W, ref, B, L, Nq, dt, kv_len=kv)
        assert torch.equal(_bits(run.loss[1:2]), _bits(same.loss[1:2])) and torch.equal(_bits(run.out_g), _bits(same.out_g)), what


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_g_loss_scales_exactly_for_a_power_of_two(dt):
    B, L, Nq, V, H = 2, 72, 8, 528, 256
    one = _random_case(B, L, Nq, V, H, dt, seed=21)
    for gl in (0.125, 4.0):
        run = _random_case(B, L, Nq, V, H, dt, seed=21, g_loss=gl)
        check_against_f64(run, f"g_loss {gl} {dt}")
        assert torch.equal(run.out_g.float(), one.out_g.float() * gl)
        assert torch.equal(_bits(run.loss[1:2]), _bits(one.loss[1:2]))
    f16g = _random_case(B, L, Nq, V, H, dt, seed=21, gdt=F16, g_loss=256.0)  # an fp16 gradient buffer is written as fp16
    check_against_f64(f16g, f"fp16 g_out {dt}")


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_two_launches_are_bit_identical(dt):
    run = _random_case(4, 256, 16, 8192 + 16, 512, dt, seed=33)  # two vocabulary chunks, ragged last tile
    assert run.rc_f == 0 and run.rc_b == 0
    first = [t.clone() for t in (run.loss, run.count, run.lse, run.row_loss, run.pG.buf)]
    run.ws.fill_(0x5A)  # (whatever an earlier call left in the workspace must not matter)
    run.rerun()
    for a, b in zip(first, (run.loss, run.count, run.lse, run.row_loss, run.pG.buf)):
        assert torch.equal(_bits(a) if a.dtype != torch.int32 else a, _bits(b) if b.dtype != torch.int32 else b)


def test_workspace_is_bounded_and_checked():
    capi = _capi()
    need = capi.lib().tcavt_lm_loss_workspace_bytes(8192, 128256, 2048)
    assert 0 < need <= CAP, need
    assert need < 8192 * 128256  # not even one byte per logit
    print(f"[lm_loss] workspace at rows 8192, V 128256, H 2048: {need / MIB:.1f} MiB (cap 640 MiB; fp32 logits: {8192 * 128256 * 4 / MIB:.0f} MiB)")
    g = torch.Generator().manual_seed(1)
    B, L, Nq, V, H = 2, 40, 8, 528, 256
    h, W = torch.randn(B * L, H, generator=g).double(), torch.randn(V, H, generator=g).double()
    small = LmRun(h, W, _labels(B, L - Nq, V, g), B, L, Nq, BF16, ws_bytes=capi.lib().tcavt_lm_loss_workspace_bytes(B * L, V, H) - 256)
    assert small.rc_f == 1 and b"workspace too small" in capi.lib().tcavt_last_error()
    assert torch.isnan(small.loss).all() and (small.count == -12345).all()  # refused before anything ran


def test_peak_memory_of_a_full_vocabulary_call():
    """Peak allocation of forward + backward at V = 128256 stays under the workspace cap + the outputs: no [rows, V] array."""
    from tcavt_amd import ops

    dev = torch.device("cuda")
    B, L, Nq, V, H = 8, 256, 16, 128256, 2048
    g = torch.Generator().manual_seed(2)
    table = (torch.randn(V, H, generator=g) / 8).to(F16).to(dev)
    table_t = ops.lm_table_t(table)
    h16 = torch.randn(B * L, H, generator=g).to(F16).to(dev)
    labels = _labels(B, L - Nq, V, g).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ws = torch.empty(ops.lm_loss_workspace_bytes(B * L, V, H), dtype=torch.uint8, device=dev)
    loss, count = torch.empty(1, dtype=F32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    lse, g_out = torch.empty(B * L, dtype=F32, device=dev), torch.empty(B * L, H, dtype=BF16, device=dev)
    ops.lm_loss_forward(h16, table, labels, Nq, B, L, loss=loss, count=count, lse=lse, workspace=ws)
    ops.lm_loss_backward(h16, table, table_t, labels, Nq, B, L, lse=lse, count=count, g_out=g_out, workspace=ws)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    outputs = g_out.numel() * 2 + lse.numel() * 4 + 1024
    assert peak <= CAP + outputs, peak
    assert peak < B * L * V  # far below even a one-byte-per-logit array
    assert torch.isfinite(loss).all() and int(count) == int((labels != -100).sum())


def test_report_worst_ratio():
    """(pytest -s) the worst measured accumulator ratios per case: what _C_ACC / _C_BWD are set against."""
    for k, (f, b) in sorted(_WORST.items()):
        print(f"[lm_loss] worst c  {k:40s} forward {f:.3f}  backward {b:.3f}")
    assert all(f <= _C_ACC and b <= _C_BWD for f, b in _WORST.values())
