"""tcavt_lm_eval through the C entry point against float64, in fp16 and bf16.

Construction, reference and bounds are those of tests/test_lm_loss_gpu.py (imported, not copied): the operands are rounded
to the 16-bit type once, the reference is float64 on the GPU from the SAME operands, outputs live inside larger NaN /
sentinel-filled buffers, and the inputs must be bit-unchanged after the call.

  loss, count, lse, row_loss : bit-identical to tcavt_lm_loss_forward on the same buffers
  pred                       : inside the plausible set {v : z64_v + b_v >= max_u (z64_u - b_u)}, b_v = _C_ACC * U * A[row, v]
                               (the forward accumulator bound of the LM-loss tests); where the set has one member, that one.
                               At most 1 % of the rows may have more than one member
  correct, sample_tokens, sample_correct : exact integers given pred
  sample_nll                 : 1e-6 relative of the float64 sum of row_loss (fp64 partial sums, one fp32 rounding: 6e-8)
  unlabelled rows            : pred -1; a sample without labels reads 0 / 0 / 0
"""
import ctypes

import pytest
import torch

from tests.test_lm_loss_gpu import (BF16, CAP, F16, F32, MIB, U, _C_ACC, LmRun, _bits, _capi, _labels, _random_case,
                                    expected_targets)

pytestmark = pytest.mark.gpu

SENT = -12345
DTS = pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])


class EvalRun:
    """tcavt_lm_eval on the input buffers of an LmRun (whose forward has run: the bits to match)."""

    def __init__(self, fwd, ws_bytes=None):
        capi = _capi()
        dev = torch.device("cuda")
        self.fwd = fwd
        B, R = fwd.B, fwd.R
        nan = float("nan")
        self.loss = torch.full((4,), nan, dtype=F32, device=dev)
        self.lse = torch.full((R + 8,), nan, dtype=F32, device=dev)
        self.row_loss = torch.full((R + 8,), nan, dtype=F32, device=dev)
        self.sample_nll = torch.full((B + 8,), nan, dtype=F32, device=dev)
        self.count = torch.full((4,), SENT, dtype=torch.int32, device=dev)
        self.correct = torch.full((4,), SENT, dtype=torch.int32, device=dev)
        self.flag = torch.zeros(4, dtype=torch.int32, device=dev)
        self.pred = torch.full((R + 8,), SENT, dtype=torch.int32, device=dev)
        self.sample_tokens = torch.full((B + 8,), SENT, dtype=torch.int32, device=dev)
        self.sample_correct = torch.full((B + 8,), SENT, dtype=torch.int32, device=dev)
        self.ws_need = capi.lib().tcavt_lm_eval_workspace_bytes(R, fwd.V, fwd.H)
        self.ws = torch.full((self.ws_need if ws_bytes is None else ws_bytes,), 0xFF, dtype=torch.uint8, device=dev)
        a = capi.LmEvalArgs()
        a.h16, a.ldh, a.table = fwd.pH.buf.data_ptr(), fwd.pH.ld, fwd.pW.buf.data_ptr()
        a.labels = fwd.labels.data_ptr()
        a.kv_len = None if fwd.kv_len is None else fwd.kv_len.data_ptr()
        a.B, a.L, a.V, a.H, a.Nq = B, fwd.L, fwd.V, fwd.H, fwd.Nq
        a.dtype16 = capi.F16 if fwd.dt == F16 else capi.BF16
        a.loss, a.count, a.lse = self.loss[1:].data_ptr(), self.count[1:].data_ptr(), self.lse[4:].data_ptr()
        a.row_loss, a.flag = self.row_loss[4:].data_ptr(), self.flag[1:].data_ptr()
        a.pred, a.correct = self.pred[4:].data_ptr(), self.correct[1:].data_ptr()
        a.sample_tokens, a.sample_correct = self.sample_tokens[4:].data_ptr(), self.sample_correct[4:].data_ptr()
        a.sample_nll = self.sample_nll[4:].data_ptr()
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), self.ws.numel()
        self.args = a
        self.rc = capi.lib().tcavt_lm_eval(ctypes.byref(a), capi.stream_ptr())
        torch.cuda.synchronize()

    def outputs(self):
        return (self.loss, self.count, self.lse, self.row_loss, self.pred, self.correct, self.sample_tokens, self.sample_correct,
                self.sample_nll, self.flag)

    def rerun(self):
        capi = _capi()
        assert capi.lib().tcavt_lm_eval(ctypes.byref(self.args), capi.stream_ptr()) == 0
        torch.cuda.synchronize()

    @property
    def out_pred(self):
        return self.pred[4:4 + self.fwd.R]

    def check_buffers(self, what):
        f = self.fwd
        f.pH.check_unchanged(f"{what}: h16")
        f.pW.check_unchanged(f"{what}: table")
        assert torch.equal(f.labels, f.labels0), f"{what}: labels changed"
        if f.kv_len is not None:
            assert torch.equal(f.kv_len, f.kv0)
        assert torch.isnan(self.loss[0]) and torch.isnan(self.loss[2:]).all(), f"{what}: write around loss"
        for t, n in ((self.count, "count"), (self.correct, "correct")):
            assert t[0] == SENT and (t[2:] == SENT).all(), f"{what}: write around {n}"
        assert self.flag[0] == 0 and (self.flag[2:] == 0).all(), f"{what}: write around flag"
        for t, n, k in ((self.lse, "lse", f.R), (self.row_loss, "row_loss", f.R), (self.sample_nll, "sample_nll", f.B)):
            assert torch.isnan(t[:4]).all() and torch.isnan(t[4 + k:]).all(), f"{what}: write around {n}"
            assert torch.isfinite(t[4:4 + k]).all(), f"{what}: {n} not finite"
        for t, n, k in ((self.pred, "pred", f.R), (self.sample_tokens, "sample_tokens", f.B), (self.sample_correct, "sample_correct", f.B)):
            assert (t[:4] == SENT).all() and (t[4 + k:] == SENT).all(), f"{what}: write around {n}"
            assert (t[4:4 + k] != SENT).all(), f"{what}: {n} not written"


def check_eval(ev, what, f64=True):
    """Everything the module docstring lists; returns (targets by row, number of rows with an ambiguous arg-max)."""
    f = ev.fwd
    dev = f.pH.buf.device
    assert f.rc_f == 0 and ev.rc == 0, _capi().lib().tcavt_last_error()
    ev.check_buffers(what)
    B, L, R, V = f.B, f.L, f.R, f.V
    # the loss outputs: the forward's bits
    assert torch.equal(_bits(ev.loss[1:2]), _bits(f.loss[1:2])), f"{what}: loss bits differ from tcavt_lm_loss_forward"
    assert torch.equal(ev.count[1:2], f.count[1:2]) and ev.flag[1] == f.flag[1], f"{what}: count / flag"
    assert torch.equal(_bits(ev.lse[4:4 + R]), _bits(f.out_lse)), f"{what}: lse bits differ"
    assert torch.equal(_bits(ev.row_loss[4:4 + R]), _bits(f.out_row_loss)), f"{what}: row_loss bits differ"
    tgt, bad = expected_targets(f.labels, B, L, f.Nq, V, f.kv_len)
    tgt = tgt.to(dev)
    assert int(ev.flag[1]) == int(bad) and int(ev.count[1]) == int((tgt >= 0).sum())
    pred = ev.out_pred.long()
    lab = tgt >= 0
    assert (pred[~lab] == -1).all(), f"{what}: unlabelled rows must read -1"
    assert ((pred[lab] >= 0) & (pred[lab] < V)).all(), f"{what}: pred outside [0, V)"
    ambiguous = 0
    if f64:
        rows = torch.nonzero(lab).flatten()
        W = f.pW.region.double()
        Wabs = W.abs()
        blk = max(16, min(256, (1 << 25) // V))
        for i in range(0, rows.numel(), blk):
            r = rows[i:i + blk]
            h = f.pH.region[r].double()
            z = h @ W.T
            b = _C_ACC * U * (h.abs() @ Wabs.T)
            plausible = (z + b) >= (z - b).max(dim=1, keepdim=True).values
            n = plausible.sum(dim=1)
            ambiguous += int((n > 1).sum())
            assert plausible.gather(1, pred[r][:, None]).all(), f"{what}: pred outside the plausible set"
            one = n == 1
            assert torch.equal(pred[r][one], z.argmax(dim=1)[one]), f"{what}: pred differs from the float64 arg-max"
            del z, b, plausible
        assert ambiguous <= 0.01 * max(rows.numel(), 1), f"{what}: {ambiguous} of {rows.numel()} rows ambiguous"
    hit = (lab & (pred == tgt)).view(B, L)
    assert int(ev.correct[1]) == int(hit.sum()), f"{what}: correct"
    assert torch.equal(ev.sample_tokens[4:4 + B].long(), lab.view(B, L).sum(dim=1)), f"{what}: sample_tokens"
    assert torch.equal(ev.sample_correct[4:4 + B].long(), hit.sum(dim=1)), f"{what}: sample_correct"
    ref = ev.row_loss[4:4 + R].double().view(B, L).sum(dim=1)
    got = ev.sample_nll[4:4 + B].double()
    assert ((got - ref).abs() <= 1e-6 * ref.abs()).all(), f"{what}: sample_nll {got.tolist()} vs {ref.tolist()}"
    empty = lab.view(B, L).sum(dim=1) == 0
    assert (ev.sample_nll[4:4 + B][empty] == 0).all() and (ev.sample_tokens[4:4 + B][empty] == 0).all() \
        and (ev.sample_correct[4:4 + B][empty] == 0).all(), f"{what}: a sample without labels must read 0 / 0 / 0"
    print(f"[lm_eval] {what}: N = {int(lab.sum())}, correct = {int(ev.correct[1])}, ambiguous rows = {ambiguous}")
    return tgt, ambiguous


SHAPES = [(3, 100, 16, 528, 256), (4, 256, 16, 1024, 512), (1, 40, 16, 128256, 256)]


@DTS
@pytest.mark.parametrize("shape", SHAPES, ids=["300x528x256", "1024x1024x512", "40x128256x256"])
def test_eval_against_float64_and_forward_bits(dt, shape):
    B, L, Nq, V, H = shape
    fwd = _random_case(B, L, Nq, V, H, dt, seed=V + H, scale=4.0, backward=False)
    if B > 1:
        fwd.labels[B - 1].fill_(-100)  # one sample without labels; rerun the forward on the changed labels
        fwd.labels0 = fwd.labels.clone()
        assert _capi().lib().tcavt_lm_loss_forward(ctypes.byref(fwd.args), _capi().stream_ptr()) == 0
        torch.cuda.synchronize()
    ev = EvalRun(fwd)
    check_eval(ev, f"{B * L}x{V}x{H} {dt}")
    # two launches: identical bits in every output, whatever the workspace held
    first = [t.clone() for t in ev.outputs()]
    ev.ws.fill_(0x5A)
    ev.rerun()
    for a, b in zip(first, ev.outputs()):
        assert torch.equal(_bits(a), _bits(b))


def _all_labelled(B, L, Nq, V, g):
    return torch.randint(0, V, (B, L - Nq), generator=g)


def _labelled_rows(B, L, Nq):
    return [b * L + p for b in range(B) for p in range(Nq - 1, L - 1)]


@DTS
@pytest.mark.parametrize("shape", [(3, 100, 16, 528, 256), (7, 40, 16, 128256, 256)], ids=["V528", "V128256"])
def test_planted_winners(dt, shape):
    """h[row] is the unit vector of feature f(row), W[v*(f), f] = 8 over noise of 2^-6: the arg-max is v*(f) exactly."""
    B, L, Nq, V, H = shape
    g = torch.Generator().manual_seed(41)
    nt = (V + 127) // 128
    last = 128 * (nt - 1)
    # columns 0 .. 127 are every (j, fq, e) of a tile: all eight j blocks, four fq groups, four registers
    vstar = list(range(128)) + [V - 1, 128, 255, 256, last - 1, last, V - 16, V - 9]
    assert {0, 127, 128, V - 1} <= set(vstar) and len(vstar) <= len(_labelled_rows(B, L, Nq))
    vstar += [(f * 37 + 5) % V for f in range(len(vstar), H)]
    W = torch.randn(V, H, generator=g).double() * 2.0 ** -6
    for f, v in enumerate(vstar):
        W[v, f] = 8.0
    rows = _labelled_rows(B, L, Nq)
    h = torch.zeros(B * L, H, dtype=torch.float64)
    want = torch.full((B * L,), -1, dtype=torch.int64)
    for k, r in enumerate(rows):
        h[r, k % H] = 1.0
        want[r] = vstar[k % H]
    assert set(vstar[:136]) <= set(want.tolist())
    fwd = LmRun(h, W, _all_labelled(B, L, Nq, V, g), B, L, Nq, dt, backward=False)
    ev = EvalRun(fwd)
    check_eval(ev, f"planted V {V} {dt}", f64=False)
    assert torch.equal(ev.out_pred.long().cpu(), want)


@DTS
def test_exact_ties_take_the_lowest_column(dt):
    """Bitwise-equal table rows that are both the row's maximum: same lane (other register, other j block), other lane of
    the tile (other fq, other j and fq), different tiles (two full ones; a full one and the ragged one; first and last)."""
    B, L, Nq, V, H = 2, 72, 8, 528, 256
    pairs = [(4, 5), (36, 52), (70, 74), (97, 123), (133, 261), (300, 520), (10, 527)]
    g = torch.Generator().manual_seed(43)
    W = torch.randn(V, H, generator=g).double() * 2.0 ** -6
    for f, (v1, v2) in enumerate(pairs):
        W[v1, f] = 8.0
        W[v2] = W[v1]
    rows = _labelled_rows(B, L, Nq)
    h = torch.randn(B * L, H, generator=g).double() * 2.0 ** -6
    want = torch.full((B * L,), -1, dtype=torch.int64)
    for k, r in enumerate(rows):
        h[r, : len(pairs)] = 0.0
        h[r, k % len(pairs)] = 1.0
        want[r] = pairs[k % len(pairs)][0]
    fwd = LmRun(h, W, _all_labelled(B, L, Nq, V, g), B, L, Nq, dt, backward=False)
    for v1, v2 in pairs:
        assert torch.equal(_bits(fwd.pW.region[v1]), _bits(fwd.pW.region[v2]))
    ev = EvalRun(fwd)
    check_eval(ev, f"ties {dt}", f64=False)
    assert torch.equal(ev.out_pred.long().cpu(), want)


@DTS
def test_masked_columns_never_win(dt):
    """V = 528, every valid logit near -60: the zero-filled table rows of the ragged tile would score 0."""
    B, L, Nq, V, H = 2, 72, 8, 528, 256
    g = torch.Generator().manual_seed(47)
    W = torch.zeros(V, H, dtype=torch.float64)
    W[:, 0] = -60.0 + torch.rand(V, generator=g).double()
    h = torch.zeros(B * L, H, dtype=torch.float64)
    h[:, 0] = 1.0
    fwd = LmRun(h, W, _all_labelled(B, L, Nq, V, g), B, L, Nq, dt, backward=False)
    ev = EvalRun(fwd)
    tgt, _ = check_eval(ev, f"masked {dt}", f64=False)  # (rounded to 16 bits the valid logits tie: z_v = W[v, 0] exactly)
    p = ev.out_pred[tgt >= 0]
    assert ((p >= 0) & (p < V)).all()
    col = fwd.pW.region[:, 0].double()
    assert (p.long() == int(torch.nonzero(col == col.max())[0])).all()  # the lowest column among the equal maxima


@DTS
def test_semantics_shift_last_position_and_kv_len(dt):
    B, L, Nq, V, H = 3, 40, 16, 528, 256
    g = torch.Generator().manual_seed(5)
    lab = _labels(B, L - Nq, V, g, frac=0.5)
    lab[:, 0] = torch.tensor([17, -100, 400])  # the last image row (p = Nq - 1) predicts labels[:, 0]
    lab[:, -1] = torch.tensor([3, 4, -100])
    lab[2, L - Nq - 6:] = -100
    kv = torch.tensor([L, L, L - 6])
    h = torch.randn(B * L, H, generator=g).double()
    W = (torch.randn(V, H, generator=g) / 4).double()
    ev = EvalRun(LmRun(h, W, lab, B, L, Nq, dt, kv_len=kv, backward=False))
    check_eval(ev, f"semantics {dt}")
    pred = ev.out_pred.view(B, L)
    assert pred[0, Nq - 1] >= 0 and pred[1, Nq - 1] == -1 and pred[2, Nq - 1] >= 0
    assert (pred[:, : Nq - 1] == -1).all() and (pred[:, L - 1] == -1).all()
    assert pred[0, L - 2] >= 0 and pred[2, L - 2] == -1


@DTS
def test_no_labelled_row(dt):
    B, L, Nq, V, H = 2, 40, 8, 528, 256
    g = torch.Generator().manual_seed(6)
    h = torch.randn(B * L, H, generator=g).double()
    W = torch.randn(V, H, generator=g).double()
    ev = EvalRun(LmRun(h, W, torch.full((B, L - Nq), -100, dtype=torch.int64), B, L, Nq, dt, backward=False))
    check_eval(ev, f"N = 0 {dt}")
    assert int(ev.count[1]) == 0 and int(ev.correct[1]) == 0 and torch.isnan(ev.loss[1])
    assert (ev.out_pred == -1).all()


@DTS
def test_bad_labels_set_the_flag_and_drop_the_row(dt):
    B, L, Nq, V, H = 2, 40, 8, 528, 256
    g = torch.Generator().manual_seed(8)
    h = torch.randn(B * L, H, generator=g).double()
    W = (torch.randn(V, H, generator=g) / 4).double()
    lab = _labels(B, L - Nq, V, g, frac=0.7)
    kv = torch.tensor([L, L - 6])
    lab[1, L - Nq - 6:] = -100
    clean = EvalRun(LmRun(h, W, lab, B, L, Nq, dt, kv_len=kv, backward=False))
    check_eval(clean, f"clean {dt}")
    assert int(clean.flag[1]) == 0
    for what, (b, j, val) in {"label == V": (0, 4, V), "negative label": (0, 9, -5), "label beyond kv_len": (1, L - Nq - 3, 7)}.items():
        bad = lab.clone()
        bad[b, j] = val
        ev = EvalRun(LmRun(h, W, bad, B, L, Nq, dt, kv_len=kv, backward=False))
        check_eval(ev, f"{what} {dt}")
        assert int(ev.flag[1]) == 1 and int(ev.out_pred[b * L + Nq + j - 1]) == -1, what


def test_workspace_is_bounded_and_checked():
    lib = _capi().lib()
    need = lib.tcavt_lm_eval_workspace_bytes(8192, 128256, 2048)
    assert 0 < need < lib.tcavt_lm_loss_workspace_bytes(8192, 128256, 2048) and need < CAP
    assert need <= 16 * 8192 * 1002 + 64 * 8192  # per-tile statistics and the row arrays, nothing else
    print(f"[lm_eval] workspace at rows 8192, V 128256, H 2048: {need / MIB:.1f} MiB")
    g = torch.Generator().manual_seed(1)
    B, L, Nq, V, H = 2, 40, 8, 528, 256
    h, W = torch.randn(B * L, H, generator=g).double(), torch.randn(V, H, generator=g).double()
    fwd = LmRun(h, W, _labels(B, L - Nq, V, g), B, L, Nq, BF16, backward=False)
    small = EvalRun(fwd, ws_bytes=lib.tcavt_lm_eval_workspace_bytes(B * L, V, H) - 256)
    assert small.rc == 1 and b"workspace too small" in lib.tcavt_last_error()
    assert torch.isnan(small.loss).all() and (small.count == SENT).all() and (small.pred == SENT).all()  # refused before any launch
