"""tcavt_sample_tokens_per_request (csrc/sampler.hip: the REQ instantiations of sample_kernel and sample_slice_kernel) through
ops.sample_tokens(per_request=...): every row takes its parameters from a device table at its REQUEST INDEX -- the row in the
batch form, out_row[slot] in the slots and rows forms.

  1. every row against the float64 reference of tests/sampler_ref.py with ITS OWN parameters (cases: tests/per_request_cases.py;
     tests/test_per_request_reference_cpu.py shows that the reference alone leaves at most 2 % of them undecided): decided cases
     exactly, undecided ones among the alternatives, the processed logits, every state array, the sentinel bands;
  2. a table of identical entries equals tcavt_sample_tokens with that struct, bit for bit, ending rules set;
  3. per-request min_new_tokens and EOS: a row's ban pattern is stop_util.ban_scores with its own values, and a row ends on its own
     EOS only;
  4. a request index outside the table: the row is inert, the flag is set, nothing else changes.
"""
import numpy as np
import pytest
import torch

from tests import per_request_cases as PC
from tests import sampler_ref as SR
from tests.stop_util import ban_scores
from tests.test_sampler_float64_gpu import Band

pytestmark = pytest.mark.gpu

PAD = PC.PAD
STAGES = pytest.mark.parametrize("two_stage", [False, True], ids=["one-stage", "two-stage"])
FORMS = pytest.mark.parametrize("form", PC.FORMS)
OUT_CAP = 16


def _struct(capi, q):
    return capi.SampleParams(q["T"], q["p"], q["rep"], q["k"], q["ngram"], q["do_sample"], q["eos"], PAD, q["seed"])


class Table:
    """An uploaded ops.RequestTable whose arrays are re-homed inside sentinel bands; ``poison`` valid-looking entries (greedy, pad
    as EOS) stand on either side of the table, so that a read beyond it shows as a row that is not inert, not as a fault."""

    def __init__(self, dev, prm, mins=None, has_stop=False, poison=2):
        from tcavt_amd import capi, ops

        self.rt = ops.RequestTable([_struct(capi, q) for q in prm], mins, has_stop_bitmap=has_stop).to(dev)
        n, size = len(prm), 48
        assert self.rt.table.numel() == n * size
        bad = torch.frombuffer(bytearray(bytes(capi.SampleParams(1.0, 1.0, 1.0, 1, 0, 0, PAD, PAD, 0))), dtype=torch.uint8)
        whole = torch.cat([bad.repeat(poison), self.rt.table.cpu(), bad.repeat(poison)])
        self.band = Band(whole, dev, fill=0xEE)
        self.whole = whole
        self.rt.table = self.band.t[poison * size:(poison + n) * size]
        self.min_band = None
        if mins is not None:
            self.min_band = Band(torch.tensor(mins, dtype=torch.int32), dev)
            self.rt.min_new = self.min_band.t
        self.flag_band = Band(torch.zeros(1, dtype=torch.int32), dev)
        self.rt.flag = self.flag_band.t
        self.rt._struct = None

    def check(self):
        self.band.check("table")
        assert torch.equal(self.band.t.cpu(), self.whole), "the table changed"
        if self.min_band is not None:
            self.min_band.check("min_new_tokens")
        self.flag_band.check("bad_index_flag")

    def flag(self):
        return int(self.flag_band.t.item())


class Harness:
    """One input set on the device in one of the three forms; call() resets the state, runs one sampler step and returns what it
    left.  Logits rows and state entries are eight each; out_tokens has n_req rows (one per row in the batch form)."""

    def __init__(self, dev, form, two_stage, scores, hist, hl, steps, out_row=None, slot_of_row=None, max_new=None, n_req=PC.N_REQ):
        from tcavt_amd import capi, ops

        self.capi, self.ops, self.dev, self.form = capi, ops, dev, form
        self.R, self.V = scores.shape
        self.cap = hist.shape[1]
        R = self.R
        self.logits = Band(torch.from_numpy(scores), dev, fill=7777.0)
        self.hist = Band(torch.from_numpy(hist), dev)
        self.hist_len = Band(torch.from_numpy(hl.astype(np.int32)), dev)
        self.cur = Band(torch.full((R,), -5, dtype=torch.int64), dev)
        self.pos = Band(torch.arange(R, dtype=torch.int32) + 100, dev)
        self.fin = Band(torch.zeros(R, dtype=torch.int32), dev)
        self.out = Band(torch.full((R if form == "batch" else n_req, OUT_CAP), -1, dtype=torch.int64), dev)  # (batch: request = row)
        self.step = Band(torch.as_tensor(np.atleast_1d(np.asarray(steps, dtype=np.int32))), dev)
        self.bands = {k: getattr(self, k) for k in ("logits", "hist", "hist_len", "cur", "pos", "fin", "out", "step")}
        self.fixed = {}
        if form != "batch":
            self.fixed["max_new"] = Band(torch.as_tensor(np.asarray(max_new if max_new is not None else [20] * R, dtype=np.int32)), dev)
            self.fixed["out_row"] = Band(torch.as_tensor(np.asarray(out_row, dtype=np.int64)), dev)
        if form == "rows":
            self.fixed["slot_of_row"] = Band(torch.as_tensor(np.asarray(slot_of_row, dtype=np.int32)), dev)
        self.ws = None
        if two_stage:
            assert self.V % 4 == 0
            self.ws = Band(torch.zeros(int(capi.lib().tcavt_sample_workspace_bytes(R)), dtype=torch.uint8), dev, fill=0xA5)

    def call(self, sp, table=None, fin=None, stop=None):
        for b in self.bands.values():
            b.reset()
        if fin is not None:
            self.fin.t.copy_(torch.from_numpy(np.asarray(fin, dtype=np.int32)))
        f = {k: b.t for k, b in self.fixed.items()}
        self.ops.sample_tokens(self.logits.t, self.hist.t, self.hist_len.t, sp, self.step.t, self.cur.t, self.pos.t, self.fin.t,
                               self.out.t, advance_pos=True, workspace=None if self.ws is None else self.ws.t,
                               max_new=f.get("max_new"), out_row=f.get("out_row"), slot_of_row=f.get("slot_of_row"), stop=stop,
                               per_request=None if table is None else table.rt)
        torch.cuda.synchronize()
        for nm, b in list(self.bands.items()) + list(self.fixed.items()):
            b.check(nm)
        for nm, b in self.fixed.items():
            assert torch.equal(b.t, b.base), f"{nm} changed"
        if self.ws is not None:
            self.ws.check("workspace")
            assert int(self.ws.t[:64 + 4 * self.R].sum().item()) == 0, "ticket / overflow words not back to zero"
        if table is not None:
            table.check()
        return {k: b.np() for k, b in self.bands.items()}


def _neutral(capi):
    """The call's own struct: it carries the pad token; the rest is what a call without a table would use."""
    return capi.SampleParams(1.0, 1.0, 1.0, 1, 0, 0, -1, PAD, 0)


def _expect(h, place, toks, ends, fin0, hist, hl, steps):
    """The state a step leaves.  place: (row, entry, request, step) of the rows that take part; toks / ends: per entry, the token a
    live entry chose and whether it ends with it; everything else keeps its initial value."""
    R = h.R
    batch = h.form == "batch"
    out = np.full((h.out.t.shape[0], OUT_CAP), -1, dtype=np.int64)
    h2, l2, fin2 = hist.copy(), hl.copy().astype(np.int32), np.asarray(fin0, dtype=np.int32).copy()
    cur, pos = np.full(R, -5, dtype=np.int64), np.arange(R, dtype=np.int32) + 100
    st2 = np.atleast_1d(np.asarray(steps, dtype=np.int32)).copy()
    for _, e, req, step in place:
        if fin0[e]:
            cur[e] = PAD
            if not batch:
                continue
        t = PAD if fin0[e] else toks[e]
        if step < OUT_CAP:
            out[req, step] = t
        cur[e], h2[e, hl[e]], l2[e], pos[e] = t, t, hl[e] + 1, pos[e] + 1
        if not batch:
            st2[e] = step + 1
        if not fin0[e]:
            fin2[e] = int(ends[e])
    if batch:
        st2[0] += 1
    return dict(out=out, cur=cur, hist=h2, hist_len=l2, pos=pos, fin=fin2, step=st2)


def _layout(form, steps=None):
    if form == "batch":
        return dict(steps=[0])
    return dict(steps=PC.STEPS if steps is None else steps, out_row=PC.OUT_ROW, slot_of_row=PC.SLOT_OF_ROW if form == "rows" else None)


# ------------------------------------------------------------------------------------------------
# 1. every row under its own parameters, against float64
# ------------------------------------------------------------------------------------------------
@STAGES
@FORMS
@pytest.mark.parametrize("V", PC.VOCABS)
def test_every_row_follows_its_own_parameters(gpu, V, form, two_stage):
    """Eight rows, ten requests, per request its own (T, top_k, top_p, repetition_penalty, no_repeat_ngram_size, do_sample, seed);
    slots: out_row is a permutation that is not the identity and the slots stand at mixed steps, slot 1 reaches its budget; rows:
    one logits row has no slot (its logits stay bit for bit).  Held to sampler_ref.Reference(...).choose(..., row = request)."""
    scores, hist, hl = PC.inputs(V)
    lay = _layout(form)
    mx = np.array([20, 4, 20, 20, 20, 20, 20, 20], dtype=np.int32)
    h = Harness(gpu["device"], form, two_stage, scores, hist, hl, max_new=mx, **lay)
    tally = SR.Tally(f"per-request V={V} {form} {'two' if two_stage else 'one'}-stage")
    fin0 = PC.FIN0  # one finished entry among the live ones
    for j in PC.calls(V):
        cases = PC.choices(V, form, j)
        if form == "batch":
            h.step.base.fill_(cases[0][3])
        table = Table(gpu["device"], PC.request_params(j))
        res = h.call(_neutral(h.capi), table, fin=fin0)
        assert table.flag() == 0
        toks, ends = {}, {}
        for row, e, req, step, q, ref, choice in cases:
            tally.processed(ref, res["logits"][row])  # (the processors run on finished rows too)
            if fin0[e]:
                continue
            toks[e] = int(res["hist"][e, hl[e]])
            tally.token(choice, toks[e], (V, form, j, row, e, req, q))
            ends[e] = form != "batch" and step + 1 == mx[e]
        want = _expect(h, [c[:4] for c in cases], toks, ends, fin0, hist, hl, h.step.base.cpu().numpy())
        for nm, w in want.items():
            assert np.array_equal(res[nm], w), (nm, j)
        if form == "rows":
            g = int(np.flatnonzero(PC.SLOT_OF_ROW < 0)[0])
            assert np.array_equal(res["logits"][g].view(np.uint32), scores[g].view(np.uint32)), "the row without a slot was processed"
    tally.finish()


# ------------------------------------------------------------------------------------------------
# 2. identical entries: the uniform entry, bit for bit
# ------------------------------------------------------------------------------------------------
@STAGES
@FORMS
def test_identical_entries_equal_the_uniform_entry(gpu, form, two_stage):
    """tcavt_sample_tokens with one struct and ending rules (a stop set, one stop sequence, min_new_tokens = 2) against the same call
    with a table of n copies of the struct -- the minimum once from the rules, once as the table's own array of 2s."""
    from tcavt_amd.stopping import StopRules

    V, dev = 512, gpu["device"]
    scores, hist, hl = PC.inputs(V)
    top = [int(np.argmax(scores[r])) for r in (0, 7)]
    q = dict(T=0.9, k=40, p=0.9, rep=1.3, ngram=3, do_sample=1, seed=(1 << 40) + 21, eos=top[1])
    seq = [int(hist[5, 29]), int(np.argmax(scores[5]))]
    for step0 in (1, 3):  # (below and above the minimum)
        lay = _layout(form, steps=np.minimum(PC.STEPS, 4) if step0 == 1 else PC.STEPS + 2)
        if form == "batch":
            lay["steps"] = [step0]
        h = Harness(dev, form, two_stage, scores, hist, hl, **lay)
        sp = _struct(h.capi, q)
        got = []
        for mode in ("uniform", "table", "table+mins"):
            m_rules = 0 if mode == "table+mins" else 2
            dr = StopRules(V, stop_token_ids=[top[0], 3], stop_sequences=[seq], min_new_tokens=m_rules).to(dev).records(PC.N_REQ, dev)
            table = None
            if mode != "uniform":
                table = Table(dev, [q] * PC.N_REQ, mins=[2] * PC.N_REQ if mode == "table+mins" else None, has_stop=True)
            res = h.call(sp, table, stop=dr)
            res["finish_reason"], res["n_generated"] = dr.finish_reason.cpu().numpy(), dr.n_generated.cpu().numpy()
            got.append(res)
            assert table is None or table.flag() == 0
        for other, mode in zip(got[1:], ("table", "table+mins")):
            for nm, a in got[0].items():
                assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, other[nm].view(np.uint32) if a.dtype == np.float32 else other[nm]), (nm, mode, step0)
        if step0 == 1:  # (the rules were live: something was banned)
            assert np.isneginf(got[0]["logits"][:, top[0]]).any()


# ------------------------------------------------------------------------------------------------
# 3. per-request minimum and EOS
# ------------------------------------------------------------------------------------------------
@STAGES
@FORMS
def test_per_request_minimum_and_eos(gpu, form, two_stage):
    """Every entry at step 2, greedy, no other processor; request r has the minimum (0, 1, 3, 5)[r % 4] and the EOS (A, B)[r % 2];
    the stop set is {C}.  The scores put A first, C second, B third in every row.  A row's processed logits are
    stop_util.ban_scores of its raw row with ITS minimum and ITS EOS; a request with EOS A and a minimum <= 2 chooses A and ends
    (reason 1); with a minimum > 2 it chooses B (A and C banned) and runs on; a request with EOS B chooses A -- its neighbour's
    EOS -- and runs on."""
    from tcavt_amd.stopping import StopRules

    V, dev, step = 512, gpu["device"], 2
    A, B, C = 100, 301, 477
    g = np.random.default_rng(5)
    scores = (g.standard_normal((8, V)) * 3.0).astype(np.float32)
    scores[:, A], scores[:, C], scores[:, B] = 50.0, 45.0, 40.0
    _, hist, hl = PC.inputs(V)
    minima, eos = [(0, 1, 3, 5)[r % 4] for r in range(PC.N_REQ)], [(A, B)[r % 2] for r in range(PC.N_REQ)]
    prm = [dict(T=1.0, k=1, p=1.0, rep=1.0, ngram=0, do_sample=0, seed=0, eos=eos[r]) for r in range(PC.N_REQ)]
    lay = _layout(form, steps=np.full(8, step, dtype=np.int32))
    if form == "batch":
        lay["steps"] = [step]
    h = Harness(dev, form, two_stage, scores, hist, hl, **lay)
    dr = StopRules(V, stop_token_ids=[C]).to(dev).records(PC.N_REQ, dev)
    table = Table(dev, prm, mins=minima, has_stop=True)
    res = h.call(_neutral(h.capi), table, stop=dr)
    assert table.flag() == 0
    place = PC.placement(form, 0)
    place = [(row, e, req, step) for row, e, req, _ in place]
    toks, ends = {}, {}
    reason, n_gen = np.zeros(PC.N_REQ, dtype=np.int32), np.zeros(PC.N_REQ, dtype=np.int32)
    for row, e, req, _ in place:
        x = ban_scores(scores[row], step, minima[req], eos[req], [C])
        assert np.array_equal(res["logits"][row].view(np.uint32), x.view(np.uint32)), ("ban pattern", row, req, minima[req], eos[req])
        toks[e] = int(np.argmax(x))
        assert toks[e] == (A if minima[req] <= step or eos[req] == B else B)
        ends[e] = toks[e] == eos[req]
        if ends[e]:
            reason[req], n_gen[req] = 1, step + 1
    assert any(ends.values()) and not all(ends.values())
    assert any(toks[e] == A and not ends[e] for e in toks), "no row chose its neighbour's EOS"
    want = _expect(h, place, toks, ends, np.zeros(8, dtype=np.int32), hist, hl, h.step.base.cpu().numpy())
    for nm, w in want.items():
        assert np.array_equal(res[nm], w), nm
    assert np.array_equal(dr.finish_reason.cpu().numpy(), reason) and np.array_equal(dr.n_generated.cpu().numpy(), n_gen)


# ------------------------------------------------------------------------------------------------
# 4. a request index outside the table
# ------------------------------------------------------------------------------------------------
@STAGES
@pytest.mark.parametrize("form", ["slots", "rows"])
def test_a_request_index_outside_the_table_is_inert(gpu, form, two_stage):
    """out_row = n_req in one slot and -1 in another: both rows write nothing -- no state, no out_tokens element, their logits stay
    bit for bit -- and bit 0 of the flag is set; every other row is as in the call where the two slots name legal requests.  The
    table stands between valid-looking entries inside a guarded allocation: a read beyond it would make the row live."""
    V, dev = 512, gpu["device"]
    scores, hist, hl = PC.inputs(V)
    prm = PC.request_params(4)
    bad = {2: PC.N_REQ, 5: -1}  # slot -> out_row
    orow_bad = PC.OUT_ROW.copy()
    for s, v in bad.items():
        orow_bad[s] = v
    res = {}
    for name, orow in (("legal", PC.OUT_ROW), ("bad", orow_bad)):
        h = Harness(dev, form, two_stage, scores, hist, hl, steps=PC.STEPS, out_row=orow, slot_of_row=PC.SLOT_OF_ROW if form == "rows" else None)
        table = Table(dev, prm)
        res[name] = h.call(_neutral(h.capi), table)
        assert table.flag() == (1 if name == "bad" else 0), name
    row_of = {int(s): g for g, s in enumerate(PC.SLOT_OF_ROW) if s >= 0} if form == "rows" else {s: s for s in range(8)}
    a, b = res["legal"], res["bad"]
    for s in range(8):
        if s in bad:
            assert b["cur"][s] == -5 and b["pos"][s] == 100 + s and b["fin"][s] == 0 and b["step"][s] == PC.STEPS[s]
            assert b["hist_len"][s] == hl[s] and np.array_equal(b["hist"][s], hist[s])
            assert np.array_equal(b["logits"][row_of[s]].view(np.uint32), scores[row_of[s]].view(np.uint32)), "an inert row was processed"
        else:
            for nm in ("cur", "pos", "fin", "step", "hist_len", "hist"):
                assert np.array_equal(a[nm][s], b[nm][s]), (nm, s)
            if s in row_of:
                assert np.array_equal(a["logits"][row_of[s]].view(np.uint32), b["logits"][row_of[s]].view(np.uint32)), s
    legal_rows = [int(PC.OUT_ROW[s]) for s in range(8) if s not in bad]
    assert np.array_equal(a["out"][legal_rows], b["out"][legal_rows])
    others = [r for r in range(PC.N_REQ) if r not in legal_rows]
    assert (b["out"][others] == -1).all(), "an inert row wrote out_tokens"
