"""tcavt_logprob_topk inside the bracket of tcavt_logprob_begin, on synthetic rows, against the float64 reference of
tests/topk_ref.py.  The ids must EQUAL the reference (the order is decided on the fp32 inputs); the values are within the bar of
tests/logprob_ref.py of float64 and bit-equal to what tcavt_logprob_finish writes when the listed id is planted as the emitted
token.  Every tensor a launch may write sits between sentinel bands and starts as a sentinel (the workspaces as garbage); the
logits are compared byte for byte across the launches.

  shapes   V = 48 (empty slices, slices shorter than k, k up to 20 < V), 1003 (V % 4 != 0), 128 256 (the model's), a base that is
           not 16-byte aligned
  inputs   topk_ref.KINDS: 3 N(0, 1); steps of 0.5 with +-0.0 (ties across slices); all equal; all but k - 2 entries -inf; the same
           maximum at both ends of every slice and at V - 1
  forms    batch / slots with a permuted out_row / rows with skipped and out-of-range map entries; a row alone, at another row
           index and beside other rows gives the same bits; a captured graph replays to the eager bits"""
import numpy as np
import pytest
import torch

from tests import logprob_ref as LR
from tests import topk_ref as TR
from tests.test_logprob_kernels_gpu import Band

pytestmark = pytest.mark.gpu

CAP = 8  # history capacity (the histories are empty: finish then reads the planted token's score from the row)
OUT_CAP = 6
SENT_I, SENT_F = -987654321, -55.5
SHAPES = [(48, k, rows) for k in (1, 4, 20) for rows in (1, 3)] + [(1003, k, 3) for k in (5, 20)] + [
    (128256, k, rows) for k in (1, 5, 20) for rows in (1, 32)]


class Rig:
    """Logits, the state the bracket reads and every output on the device, in one of the three forms."""

    def __init__(self, dev, form, V, rows, k, n_state=None, out_rows=None, misalign=0):
        from tcavt_amd import ops

        self.ops, self.dev, self.form, self.V, self.rows, self.k = ops, dev, form, V, rows, k
        self.S = S = rows if form != "rows" else n_state
        self.out_rows = out_rows or S
        i32, i64 = torch.int32, torch.int64
        self.logits_band = Band(torch.zeros(rows * V + misalign), dev, fill=7777.0)
        self.logits = self.logits_band.t[misalign:].view(rows, V)
        assert (self.logits.data_ptr() % 16 != 0) == bool(misalign)
        self.hist = Band(torch.zeros(S, CAP, dtype=i64), dev)
        self.hist_len = Band(torch.zeros(S, dtype=i32), dev)
        self.step_w = Band(torch.zeros(1 if form == "batch" else S, dtype=i32), dev)
        self.fin = Band(torch.zeros(S, dtype=i32), dev)
        self.out = Band(torch.full((self.out_rows, OUT_CAP), -1, dtype=i64), dev)
        self.out_row = Band(torch.arange(S, dtype=i64), dev) if form != "batch" else None
        self.map = Band(torch.zeros(rows, dtype=i32), dev) if form == "rows" else None
        self.tlp = Band(torch.zeros(self.out_rows, OUT_CAP), dev, fill=SENT_F)
        self.sum = Band(torch.zeros(self.out_rows), dev, fill=SENT_F)
        self.cnt = Band(torch.zeros(self.out_rows, dtype=i32), dev)
        self.lws = Band(torch.full((ops.logprob_workspace_bytes(rows, CAP),), 0x5A, dtype=torch.uint8), dev, fill=0xA5)
        self.top_ids = Band(torch.full((self.out_rows, OUT_CAP, k), SENT_I, dtype=i32), dev)
        self.top_lp = Band(torch.full((self.out_rows, OUT_CAP, k), SENT_F), dev, fill=-77.25)
        self.tws = Band(torch.full((ops.logprob_topk_workspace_bytes(rows, k),), 0x5A, dtype=torch.uint8), dev, fill=0xA5)
        self.bands = {n: v for n, v in vars(self).items() if isinstance(v, Band)}

    def args(self):
        o = self.ops
        a = o.logprob_args(self.logits, self.hist.t, self.hist_len.t, self.step_w.t, self.fin.t, self.out.t, self.tlp.t, self.sum.t,
                           self.cnt.t, self.lws.t, out_row=None if self.out_row is None else self.out_row.t,
                           slot_of_row=None if self.map is None else self.map.t)
        return a, o.logprob_topk_args(a, self.out.t, self.top_ids.t, self.top_lp.t, self.tws.t)

    def where(self):
        """[(logits row, out row, step)] of the rows that are live."""
        fin, step = self.fin.np(), self.step_w.np()
        m = self.map.np() if self.map is not None else np.arange(self.rows)
        orow = self.out_row.np() if self.out_row is not None else np.arange(self.rows)
        live = [(r, int(m[r])) for r in range(self.rows) if 0 <= m[r] < self.S and fin[m[r]] == 0]
        return [(r, int(orow[s]), int(step[0] if self.form == "batch" else step[s])) for r, s in live]

    def run(self, scores):
        """begin -> topk on fp32 [rows, V]; -> (top_ids int32 [out_rows, OUT_CAP, k], top_logprobs fp32) as numpy."""
        self.logits.copy_(torch.as_tensor(np.ascontiguousarray(scores, dtype=np.float32)))
        self.top_ids.t.fill_(SENT_I)
        self.top_lp.t.fill_(SENT_F)
        before = self.logits_band.buf.clone()
        a, ta = self.args()
        self.ops.logprob_begin(a)
        self.ops.logprob_topk(ta)
        torch.cuda.synchronize()
        assert torch.equal(self.logits_band.buf.view(torch.int32), before.view(torch.int32)), "a launch wrote logits"
        for nm, b in self.bands.items():
            b.check(nm)
        return self.top_ids.np().copy(), self.top_lp.np().copy()

    def finish_with(self, tokens_by_out_pos):
        """tcavt_logprob_finish with the given tokens planted as the emitted ones -> token_logprobs as numpy."""
        out = self.out.np().copy()
        for (o, s), tok in tokens_by_out_pos.items():
            out[o, s] = tok
        self.out.set(out)
        a, _ = self.args()
        self.ops.logprob_finish(a)
        torch.cuda.synchronize()
        return self.tlp.np().copy()


def _check(rig, scores, ids, lps, name, worst):
    """Equal ids, values within the bar, the sentinel everywhere else; then bit-equality with logprob_finish, list entry by entry."""
    k, where = rig.k, rig.where()
    mask = np.zeros(ids.shape[:2], dtype=bool)
    for r, o, s in where:
        assert not mask[o, s]
        mask[o, s] = True
        rid, rlp = TR.ref_topk(scores[r], k)
        assert ids[o, s].tolist() == rid.tolist(), f"{name}: row {r}: ids {ids[o, s].tolist()} != reference {rid.tolist()}"
        for i in range(k):
            if np.isneginf(rlp[i]):
                assert np.isneginf(lps[o, s, i]), f"{name}: row {r} entry {i}: {lps[o, s, i]!r} for a -inf score"
                continue
            q = TR.ratio(lps[o, s, i], rlp[i])
            worst[0] = max(worst[0], q)
            assert q <= 1.0, f"{name}: row {r} entry {i} id {rid[i]}: got {lps[o, s, i]!r}, reference {rlp[i]!r} ({q:.2f} of the bar)"
        assert TR.is_sorted(ids[o, s], lps[o, s]), f"{name}: row {r}: the list is not sorted"
    assert bool((ids[~mask] == SENT_I).all()) and bool((lps[~mask] == SENT_F).all()), f"{name}: written where no live row generates"
    for i in range(k):
        tlp = rig.finish_with({(o, s): int(ids[o, s, i]) for _, o, s in where})
        for _, o, s in where:
            assert tlp[o, s].tobytes() == lps[o, s, i].tobytes(), (
                f"{name}: entry {i} = {lps[o, s, i]!r} but logprob_finish writes {tlp[o, s]!r} for token {ids[o, s, i]}")


def _scores(kind, V, k, rows, seed=0):
    return np.stack([TR.make_row(kind, V, k, seed + 7 * r) for r in range(rows)])


@pytest.mark.parametrize("V,k,rows", SHAPES)
def test_every_input_kind_matches_the_reference(gpu, V, k, rows):
    dev, worst = gpu["device"], [0.0]
    rig = Rig(dev, "batch", V, rows, k)
    rig.step_w.set([2])
    for kind in TR.KINDS:
        scores = _scores(kind, V, k, rows)
        ids, lps = rig.run(scores)
        _check(rig, scores, ids, lps, f"V={V} k={k} rows={rows} {kind}", worst)
        if kind == "equal":
            assert all(ids[r, 2].tolist() == list(range(k)) for r in range(rows))
        if kind == "mostly_ninf" and k >= 3:
            x = scores[0]
            ninf = [int(i) for i in np.flatnonzero(np.isneginf(x))[:2]]
            assert ids[0, 2, k - 2:].tolist() == ninf and bool(np.isneginf(lps[0, 2, k - 2:]).all())
        if kind == "planted" and k >= 4:
            lo0, hi0 = LR.slice_bounds(V)[0]
            assert ids[0, 2, 0] == lo0 and ids[0, 2, 1] == hi0 - 1  # the tie at 50.0 goes by id, across the slices
    print(f"\n[logprob_topk] V = {V} k = {k} rows = {rows}: worst {worst[0]:.3f} of the bar")


@pytest.mark.parametrize("V,k", [(48, 20), (1003, 5), (128256, 5)])
def test_unaligned_base_takes_the_bounded_loads(gpu, V, k):
    dev, worst = gpu["device"], [0.0]
    rig = Rig(dev, "batch", V, 2, k, misalign=1)
    rig0 = Rig(dev, "batch", V, 2, k)
    for kind in ("quantised", "planted"):
        scores = _scores(kind, V, k, 2, seed=3)
        ids, lps = rig.run(scores)
        _check(rig, scores, ids, lps, f"unaligned V={V} {kind}", worst)
        ids0, lps0 = rig0.run(scores)
        assert ids.tobytes() == ids0.tobytes() and lps.tobytes() == lps0.tobytes(), "the load path changes the result"


def _by_request(ids, lps, where):
    return [(ids[o, s].tobytes(), lps[o, s].tobytes()) for o, s in where]


@pytest.mark.parametrize("V,k", [(48, 20), (1003, 5), (128256, 20)])
def test_three_forms_index_as_specified_and_a_row_is_independent_of_its_place(gpu, V, k):
    dev, worst = gpu["device"], [0.0]
    req = _scores("quantised", V, k, 3, seed=11)  # three requests
    other = _scores("normal", V, k, 6, seed=12)   # partners

    # ---- batch: rows 0, 2, 4 carry the requests, row 1 is finished, row 3 a live partner; one step word
    rig = Rig(dev, "batch", V, 5, k)
    rig.step_w.set([3])
    rig.fin.set([0, 1, 0, 0, 0])
    scores = other[:5].copy()
    scores[[0, 2, 4]] = req
    ids, lps = rig.run(scores)
    assert [(o, s) for _, o, s in rig.where()] == [(0, 3), (2, 3), (3, 3), (4, 3)]
    _check(rig, scores, ids, lps, "batch", worst)
    base = _by_request(ids, lps, [(0, 3), (2, 3), (4, 3)])

    # ---- alone: one row each
    for q in range(3):
        one = Rig(dev, "batch", V, 1, k)
        one.step_w.set([1])
        i1, l1 = one.run(req[q:q + 1])
        assert _by_request(i1, l1, [(0, 1)]) == [base[q]], "a row alone differs from the row beside others"

    # ---- slots: per-slot step words, a permuted out_row, slot 2 finished
    rig = Rig(dev, "slots", V, 5, k, out_rows=6)
    rig.step_w.set([0, 5, 9, 1, 4])
    rig.out_row.set([4, 0, 1, 2, 5])
    rig.fin.set([0, 0, 1, 0, 0])
    scores = other[:5].copy()
    scores[[1, 3, 0]] = req
    ids, lps = rig.run(scores)
    assert [(o, s) for _, o, s in rig.where()] == [(4, 0), (0, 5), (2, 1), (5, 4)]
    _check(rig, scores, ids, lps, "slots", worst)
    assert _by_request(ids, lps, [(0, 5), (2, 1), (4, 0)]) == base, "a request's lists depend on its slot or partners"
    # a step word outside [0, out_cap) writes nothing (tcavt_logprob_finish writes nothing there either)
    rig.step_w.set([0, OUT_CAP, -1, 1, 4])
    rig.fin.set([0, 0, 0, 0, 0])
    ids, lps = rig.run(scores)
    written = {(o, s) for o in range(6) for s in range(OUT_CAP) if ids[o, s, 0] != SENT_I}
    assert written == {(4, 0), (2, 1), (5, 4)}

    # ---- rows: 5 logits rows on 6 slots; row 1 has map entry -1, row 3 an entry >= S; rows 0, 2, 4 -> slots 3, 0, 5
    rig = Rig(dev, "rows", V, 5, k, n_state=6, out_rows=6)
    rig.map.set([3, -1, 0, 9, 5])
    rig.step_w.set([2, 0, 0, 0, 0, 1])
    rig.out_row.set([1, 0, 0, 5, 0, 3])
    rig.fin.set([0, 1, 1, 0, 1, 0])
    scores = other[:5].copy()
    scores[[0, 2, 4]] = req
    ids, lps = rig.run(scores)
    assert [(r, o, s) for r, o, s in rig.where()] == [(0, 5, 0), (2, 1, 2), (4, 3, 1)]
    _check(rig, scores, ids, lps, "rows", worst)
    assert _by_request(ids, lps, [(5, 0), (1, 2), (3, 1)]) == base, "a request's lists depend on its row, slot or partners"
    print(f"\n[logprob_topk] forms V = {V} k = {k}: worst {worst[0]:.3f} of the bar")


@pytest.mark.parametrize("V,k,rows", [(1003, 5, 3), (128256, 20, 8)])
def test_graph_replay_equals_eager(gpu, V, k, rows):
    dev = gpu["device"]
    rig = Rig(dev, "slots", V, rows, k)
    rig.step_w.set([r % OUT_CAP for r in range(rows)])
    scores = _scores("quantised", V, k, rows, seed=21)
    ids0, lps0 = rig.run(scores)  # eager: also the warm-up of both kernel forms
    a, ta = rig.args()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (as generation.capture does: the capture launches nothing)
        rig.ops.logprob_begin(a)
        rig.ops.logprob_topk(ta)
    # new scores in the same buffers: the replay reads them, the eager run afterwards must agree
    scores2 = _scores("quantised", V, k, rows, seed=22)
    rig.logits.copy_(torch.as_tensor(scores2))
    rig.top_ids.t.fill_(SENT_I)
    rig.top_lp.t.fill_(SENT_F)
    graph.replay()
    torch.cuda.synchronize()
    ids_g, lps_g = rig.top_ids.np().copy(), rig.top_lp.np().copy()
    for nm, b in rig.bands.items():
        b.check(nm)
    ids1, lps1 = rig.run(scores2)
    assert ids_g.tobytes() == ids1.tobytes() and lps_g.tobytes() == lps1.tobytes()
    assert ids_g.tobytes() != ids0.tobytes()
    for r in range(rows):
        assert ids_g[r, r % OUT_CAP].tolist() == TR.ref_topk(scores2[r], k)[0].tolist()
