"""tcavt_logprob_begin / tcavt_logprob_finish around the real token selection, against the float64 reference of
tests/logprob_ref.py (bar: |got - ref| <= 1e-5 + 2^-22 |ref|; derivation there).  Every tensor a launch may write sits between
sentinel bands; `logits` is compared byte for byte across the begin launch; the bracket's workspace starts as garbage.

  random grid   V in {48, 1000, 1003, 128 256, 262 144} x sigma in {1, 4, 12}, the processor pairs of sampler_ref.PROCESSORS,
                greedy and sampling; the histories hold the rows' best tokens, so a penalised token is often the one chosen
  planted rows  a wrong reading is >= 1 away: one element at 0 among -40 at the row's ends and around every slice boundary; a
                penalised token that still wins; a banned token that carries the largest mass (n-gram ban, min_new_tokens ban)
  three forms   batch / slots / rows for three consecutive steps: columns written, sum_logprob, n_scored, inert and skipped rows,
                a second run bit for bit, and the same requests at other rows / slots among other partners bit for bit

`pytest -s` prints each test's worst error in units of the bar; profiles/generate_logprobs.txt records them."""
import numpy as np
import pytest
import torch

from tests import logprob_ref as LR
from tests import sampler_ref as SR

pytestmark = pytest.mark.gpu

GUARD = 16
SENT = -987654321
PAD = 7
CAP = 40  # history capacity
OUT_CAP = 8


class Band:
    """A tensor inside a larger sentinel-filled buffer."""

    def __init__(self, init, dev, fill=SENT):
        init = torch.as_tensor(init)
        self.n, self.fill = init.numel(), fill
        self.buf = torch.full((self.n + 2 * GUARD,), fill, dtype=init.dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + self.n].view(init.shape)
        self.t.copy_(init)

    def set(self, value):
        self.t.copy_(torch.as_tensor(np.asarray(value)).to(self.t.dtype).view(self.t.shape))

    def check(self, name):
        assert bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all()), f"write around {name}"

    def np(self):
        return self.t.cpu().numpy()


class Rig:
    """Logits, the samplers' state and the three results on the device, in one of the three forms.  step() loads a set of scores,
    runs begin -> selection -> finish and returns [(out row, step, token, float64 reference)] of the rows that were live."""

    def __init__(self, dev, form, V, rows, n_state=None, out_rows=None):
        from tcavt_amd import capi, generation, ops

        self.capi, self.gen, self.ops, self.dev = capi, generation, ops, dev
        self.form, self.V, self.rows = form, V, rows
        self.S = S = rows if form != "rows" else n_state
        self.out_rows = out_rows or S
        i32, i64 = torch.int32, torch.int64
        self.logits = Band(torch.zeros(rows, V), dev, fill=7777.0)
        self.hist = Band(torch.zeros(S, CAP, dtype=i64), dev)
        self.hist_len = Band(torch.zeros(S, dtype=i32), dev)
        self.step_w = Band(torch.zeros(1 if form == "batch" else S, dtype=i32), dev)
        self.cur = Band(torch.full((S,), -5, dtype=i64), dev)
        self.pos = Band(torch.arange(S, dtype=i32) + 100, dev)
        self.fin = Band(torch.zeros(S, dtype=i32), dev)
        self.out = Band(torch.full((self.out_rows, OUT_CAP), -1, dtype=i64), dev)
        self.max_new = Band(torch.full((S,), OUT_CAP, dtype=i32), dev) if form != "batch" else None
        self.out_row = Band(torch.arange(S, dtype=i64), dev) if form != "batch" else None
        self.map = Band(torch.zeros(rows, dtype=i32), dev) if form == "rows" else None
        self.tlp = Band(torch.zeros(self.out_rows, OUT_CAP), dev, fill=-55.5)  # the host's 0.0 fill, as out's pad fill
        self.sum = Band(torch.zeros(self.out_rows), dev, fill=-55.5)
        self.cnt = Band(torch.zeros(self.out_rows, dtype=i32), dev)
        self.sws = torch.zeros(int(capi.lib().tcavt_sample_workspace_bytes(rows)), dtype=torch.uint8, device=dev)
        self.lws = Band(torch.full((ops.logprob_workspace_bytes(rows, CAP),), 0x5A, dtype=torch.uint8), dev, fill=0xA5)
        self.bands = {k: v for k, v in vars(self).items() if isinstance(v, Band)}

    def state(self):
        b = self.form == "batch"
        return self.gen.slot_state(self.hist.t, self.hist_len.t, self.step_w.t, self.cur.t, self.pos.t, self.fin.t,
                                   None if b else self.max_new.t, None if b else self.out_row.t)

    def step(self, scores, sp, stop=None):
        """scores fp32 [rows, V] -> [(out row, step, token, reference)]"""
        scores = np.ascontiguousarray(scores, dtype=np.float32)
        self.logits.set(scores)
        fin, step = self.fin.np(), self.step_w.np()
        m = self.map.np() if self.map is not None else np.arange(self.rows)
        orow = self.out_row.np() if self.out_row is not None else np.arange(self.rows)
        live = [(r, int(m[r])) for r in range(self.rows) if 0 <= m[r] < self.S and fin[m[r]] == 0]
        where = [(r, int(orow[s]), int(step[0] if self.form == "batch" else step[s])) for r, s in live]
        st = self.state()
        mp = None if self.map is None else self.map.t
        a = self.ops.logprob_args(self.logits.t, st.history, st.hist_len, st.step, st.finished, self.out.t, self.tlp.t, self.sum.t,
                                  self.cnt.t, self.lws.t, out_row=st.out_row, slot_of_row=mp)
        before = self.logits.buf.clone()
        self.ops.logprob_begin(a)
        assert torch.equal(self.logits.buf.view(torch.int32), before.view(torch.int32)), "tcavt_logprob_begin wrote logits"
        self.gen.select(self.logits.t, st, sp, self.out.t, True, self.sws, stop, slot_of_row=mp)
        self.ops.logprob_finish(a)
        torch.cuda.synchronize()
        for nm, b in self.bands.items():
            b.check(nm)
        out = self.out.np()
        res = []
        for r, o, k in where:
            tok = int(out[o, k])
            assert 0 <= tok < self.V
            res.append((o, k, tok, LR.ref_logprob(scores[r], tok)))
        return res

    def results(self):
        return self.tlp.np().copy(), self.sum.np().copy(), self.cnt.np().copy()


def _params(capi, rep=1.0, ngram=0, do_sample=0, eos=-1, seed=1234):
    return capi.SampleParams(0.9, 0.9, rep, 40, ngram, do_sample, eos, PAD, seed)


def _check(rig, scored, name, worst):
    """The three results against everything scored so far: [(out row, step, token, reference)] in launch order."""
    tlp, tot, cnt = rig.results()
    exp = np.zeros_like(tlp)
    mask = np.zeros(tlp.shape, dtype=bool)
    for o, k, tok, ref in scored:
        assert not mask[o, k]
        mask[o, k] = True
        r = LR.ratio(tlp[o, k], ref)
        worst[0] = max(worst[0], r)
        assert r <= 1.0, f"{name}: out row {o} step {k} token {tok}: got {tlp[o, k]!r}, reference {ref!r} ({r:.2f} of the bar)"
    assert np.array_equal(tlp[~mask], exp[~mask]), f"{name}: token_logprobs written where no live row emitted a token"
    for o in range(tlp.shape[0]):
        mine = [(k, ref) for oo, k, _, ref in scored if oo == o]
        assert cnt[o] == len(mine), f"{name}: n_scored[{o}]"
        run = np.float32(0.0)
        for k, _ in mine:  # (launch order = step order)
            run = np.float32(run + tlp[o, k])
        assert tot[o].tobytes() == run.tobytes(), f"{name}: sum_logprob[{o}] is not the fp32 running sum of its row"
        assert abs(float(tot[o]) - sum(ref for _, ref in mine)) <= sum(LR.bar(ref) for _, ref in mine), name


def _histories(scores, g):
    """[R, CAP] ids and lengths: random ids with the row's three best tokens among them (a penalised token that is still chosen),
    a repeated bigram at the end (an n-gram ban), one id out of range."""
    R, V = scores.shape
    hist = g.integers(0, V, size=(R, CAP)).astype(np.int64)
    hl = np.array([30, 17, 40, 3, 25][:R], dtype=np.int32)
    for r in range(R):
        n = int(hl[r])
        top = np.argsort(-scores[r].astype(np.float64), kind="stable")[:3]
        hist[r, :min(3, n)] = top[:min(3, n)]
        if n >= 8:
            hist[r, n - 1] = hist[r, 4]  # the last id occurred before: its follower hist[r, 5] is banned at n-gram size 2
            hist[r, 6] = V + 5
    return hist, hl


@pytest.mark.parametrize("V", LR.VOCABS)
def test_random_grid_is_within_the_bar(gpu, V):
    from tcavt_amd import capi

    dev = gpu["device"]
    g = np.random.default_rng(31 + V)
    sig = np.array([1.0, 4.0, 12.0, 4.0], dtype=np.float32)
    worst, n = [0.0], 0
    for rnd in range(2):
        scores = (g.standard_normal((4, V)).astype(np.float32) * np.roll(sig, rnd)[:, None]).astype(np.float32)
        hist, hl = _histories(scores, g)
        for rep, ngram in SR.PROCESSORS:
            for do_sample in (0, 1):
                rig = Rig(dev, "batch", V, 4)
                rig.hist.set(hist)
                rig.hist_len.set(hl)
                rig.step_w.set([3])
                scored = rig.step(scores, _params(capi, rep, ngram, do_sample))
                assert len(scored) == 4
                _check(rig, scored, f"V={V} rep={rep} ngram={ngram} sample={do_sample}", worst)
                n += 4
    print(f"\n[logprob] random grid V = {V}: {n} rows, worst {worst[0]:.3f} of the bar")


@pytest.mark.parametrize("V", (48, 1000, 1003, 128256, 262144))
def test_planted_single_element_at_every_boundary(gpu, V):
    from tcavt_amd import capi

    dev = gpu["device"]
    pos = LR.planted_positions(V)
    worst = [0.0]
    rig = None
    for i in range(0, len(pos), 5):
        chunk = pos[i:i + 5]
        if rig is None or rig.rows != len(chunk):
            rig = Rig(dev, "batch", V, len(chunk))
        else:
            for nm in ("tlp", "sum"):
                getattr(rig, nm).t.zero_()
            rig.cnt.t.zero_()
            rig.step_w.t.zero_()
        rig.hist_len.set([0] * len(chunk))
        scores = np.stack([LR.planted_single(V, p) for p in chunk])
        scored = rig.step(scores, _params(capi))
        assert [t for _, _, t, _ in scored] == chunk  # greedy takes the planted element
        _check(rig, scored, f"V={V} planted at {chunk}", worst)  # (a dropped element moves the result by ~ 40 - ln V)
    print(f"\n[logprob] planted single element V = {V}: {len(pos)} positions, worst {worst[0]:.3f} of the bar")


@pytest.mark.parametrize("V", (1000, 128256))
def test_planted_processor_cases_use_the_raw_row(gpu, V):
    from tcavt_amd import capi
    from tcavt_amd.stopping import StopRules

    dev = gpu["device"]
    worst = [0.0]
    for c in LR.planted_cases(V):
        rig = Rig(dev, "batch", V, 1)
        h = np.zeros((1, CAP), dtype=np.int64)
        h[0, :len(c["hist"])] = c["hist"]
        rig.hist.set(h)
        rig.hist_len.set([len(c["hist"])])
        stop = None
        if c["min_new"] > 0:  # through tcavt_sample_tokens
            stop = StopRules(V, None, None, c["min_new"]).to(dev).records(1, dev)
        scored = rig.step(c["scores"][None], _params(capi, c["penalty"], c["ngram"], 0, eos=c["eos"]), stop=stop)
        assert [t for _, _, t, _ in scored] == [c["token"]], c["name"]
        got = rig.results()[0][0, 0]
        assert abs(float(got) - c["wrong"]) >= 0.9, c["name"]
        _check(rig, scored, c["name"], worst)
        # the selection did rewrite the row in place: the raw value is no longer there to be read
        x = rig.logits.np()[0]
        changed = np.flatnonzero(x != c["scores"])
        assert changed.size >= 1, c["name"]
    print(f"\n[logprob] planted processor cases V = {V}: worst {worst[0]:.3f} of the bar")


# ---- the three forms, three consecutive steps ------------------------------------------------------------------------------
def _requests(V, n, seed):
    """n logical requests: three rows of scores (one per step), a history with the best tokens of the first row in it."""
    g = np.random.default_rng(seed)
    reqs = []
    for q in range(n):
        sc = (g.standard_normal((3, V)) * (1.0, 4.0, 12.0)[q % 3]).astype(np.float32)
        hist, hl = _histories(sc[:1], g)
        reqs.append(dict(scores=sc, hist=hist[0], hl=int((11, 30, 5, 22, 17)[q % 5])))
    return reqs


def _run_form(dev, capi, form, V, reqs, place, sp, partner_seed):
    """The requests at the rows / slots ``place`` gives them, partners (other scores, finished / skipped) everywhere else.
    -> (rig, scored by request, results by request)."""
    g = np.random.default_rng(partner_seed)
    nreq = len(reqs)
    if form == "batch":
        rows, S, out_rows = 5, 5, 5
    elif form == "slots":
        rows, S, out_rows = 5, 5, 6
    else:
        rows, S, out_rows = 5, 6, 6
    rig = Rig(dev, form, V, rows, n_state=S, out_rows=out_rows)
    hist = g.integers(0, V, size=(S, CAP)).astype(np.int64)
    hl = np.full(S, 9, dtype=np.int32)
    fin = np.zeros(S, dtype=np.int32)
    step = np.zeros(S, dtype=np.int32)
    max_new = np.full(S, OUT_CAP, dtype=np.int32)
    orow = np.zeros(S, dtype=np.int64)
    slot_of = {}  # request -> (logits row, slot)
    if form == "rows":
        mp = np.array(place["map"], dtype=np.int32)
        for q, r in enumerate(place["rows"]):
            slot_of[q] = (r, int(mp[r]))
    else:
        for q, r in enumerate(place["rows"]):
            slot_of[q] = (r, r)
    free_out = [o for o in range(out_rows) if o not in place["out_row"]]
    for s in range(S):
        orow[s] = free_out[s % len(free_out)] if free_out else 0
    for q, (r, s) in slot_of.items():
        hist[s], hl[s] = reqs[q]["hist"], reqs[q]["hl"]
        step[s] = place["step"][q]
        max_new[s] = place["max_new"][q]
        orow[s] = place["out_row"][q]
    for s in place.get("finished", ()):
        fin[s] = 1
    # (the partners that are live need out rows of their own: every live slot writes a distinct row)
    used = {int(orow[s]) for _, s in slot_of.values()}
    spare = [o for o in range(out_rows) if o not in used]
    for s in range(S):
        if s not in {s_ for _, s_ in slot_of.values()}:
            if spare and form != "batch":
                orow[s] = spare.pop()
            elif form != "batch":
                fin[s] = 1  # no row left for it: inert
    rig.hist.set(hist)
    rig.hist_len.set(hl)
    rig.fin.set(fin)
    if form == "batch":
        rig.step_w.set([place["step"][0]])
    else:
        rig.step_w.set(step)
        rig.max_new.set(max_new)
        rig.out_row.set(orow)
    if form == "rows":
        rig.map.set(mp)
    scored = []
    for k in range(3):
        scores = (g.standard_normal((rows, V)) * 3.0).astype(np.float32)
        for q, (r, s) in slot_of.items():
            scores[r] = reqs[q]["scores"][k]
        scored += rig.step(scores, sp)
    return rig, scored


def _by_out_row(rig, rows):
    tlp, tot, cnt = rig.results()
    return [(tlp[o].tobytes(), tot[o].tobytes(), cnt[o].tobytes()) for o in rows]


@pytest.mark.parametrize("V", (1003, 128256))
@pytest.mark.parametrize("do_sample", (0, 1))
def test_batch_form_three_steps(gpu, V, do_sample):
    from tcavt_amd import capi

    dev, worst = gpu["device"], [0.0]
    reqs = _requests(V, 3, 7 + V)
    sp = _params(capi, 1.3, 3, do_sample)
    # rows 0, 2, 4 carry the requests; row 1 is finished from the start, row 3 is a live partner
    place = dict(rows=[0, 2, 4], step=[2, 2, 2], max_new=[8] * 3, out_row=[0, 2, 4], finished=[1])
    rig, scored = _run_form(dev, capi, "batch", V, reqs, place, sp, 100)
    assert len(scored) == 4 * 3 and all(o != 1 for o, *_ in scored)
    assert sorted({k for _, k, *_ in scored}) == [2, 3, 4]
    _check(rig, scored, "batch", worst)
    tlp, tot, cnt = rig.results()
    assert not tlp[1].any() and tot[1] == 0 and cnt[1] == 0 and list(cnt[[0, 2, 3, 4]]) == [3] * 4
    assert bool((rig.out.t[1, 2:5] == PAD).all())  # the finished row emitted pad tokens, unscored
    rig2, scored2 = _run_form(dev, capi, "batch", V, reqs, place, sp, 100)
    assert _by_out_row(rig2, range(5)) == _by_out_row(rig, range(5)), "a second run differs"
    if not do_sample:  # (the batch form's Philox row is the logits row: only the greedy tokens are row-independent)
        place3 = dict(rows=[3, 0, 1], step=[2, 2, 2], max_new=[8] * 3, out_row=[3, 0, 1], finished=[4])
        rig3, scored3 = _run_form(dev, capi, "batch", V, reqs, place3, sp, 200)
        _check(rig3, scored3, "batch, moved", worst)
        assert _by_out_row(rig3, [3, 0, 1]) == _by_out_row(rig, [0, 2, 4]), "a row's results depend on where it runs"
    print(f"\n[logprob] batch form V = {V} sample = {do_sample}: worst {worst[0]:.3f} of the bar")


@pytest.mark.parametrize("V", (1003, 128256))
@pytest.mark.parametrize("do_sample", (0, 1))
def test_slots_form_three_steps(gpu, V, do_sample):
    from tcavt_amd import capi

    dev, worst = gpu["device"], [0.0]
    reqs = _requests(V, 3, 9 + V)
    sp = _params(capi, 1.3, 3, do_sample)
    # different step[s], a permuted out_row, and request 1 reaches its budget with its first token here (step 3 of 4)
    place = dict(rows=[0, 1, 3], step=[0, 3, 1], max_new=[8, 4, 6], out_row=[4, 0, 2], finished=[2])
    rig, scored = _run_form(dev, capi, "slots", V, reqs, place, sp, 300)
    mine = lambda o: sorted(k for oo, k, *_ in scored if oo == o)
    assert mine(4) == [0, 1, 2] and mine(0) == [3] and mine(2) == [1, 2, 3]
    _check(rig, scored, "slots", worst)
    tlp, tot, cnt = rig.results()
    assert cnt[0] == 1 and not tlp[0, :3].any() and not tlp[0, 4:].any()  # nothing after the budget: the slot is inert
    rig2, _ = _run_form(dev, capi, "slots", V, reqs, place, sp, 300)
    assert _by_out_row(rig2, range(6)) == _by_out_row(rig, range(6)), "a second run differs"
    place3 = dict(rows=[4, 2, 0], step=[0, 3, 1], max_new=[8, 4, 6], out_row=[4, 0, 2], finished=[])
    rig3, scored3 = _run_form(dev, capi, "slots", V, reqs, place3, sp, 400)
    _check(rig3, scored3, "slots, moved", worst)
    assert _by_out_row(rig3, [4, 0, 2]) == _by_out_row(rig, [4, 0, 2]), "a request's results depend on its slot or partners"
    print(f"\n[logprob] slots form V = {V} sample = {do_sample}: worst {worst[0]:.3f} of the bar")


@pytest.mark.parametrize("V", (1003, 128256))
@pytest.mark.parametrize("do_sample", (0, 1))
def test_rows_form_three_steps(gpu, V, do_sample):
    from tcavt_amd import capi

    dev, worst = gpu["device"], [0.0]
    reqs = _requests(V, 3, 11 + V)
    sp = _params(capi, 1.3, 3, do_sample)
    # 5 logits rows on 6 slots: row 1 has map entry -1, row 3 an entry >= S; rows 0, 2, 4 -> slots 3, 0, 5
    place = dict(map=[3, -1, 0, 9, 5], rows=[0, 2, 4], step=[0, 2, 1], max_new=[8, 8, 8], out_row=[5, 1, 3])
    rig, scored = _run_form(dev, capi, "rows", V, reqs, place, sp, 500)
    assert len(scored) == 9 and sorted({o for o, *_ in scored}) == [1, 3, 5]
    _check(rig, scored, "rows", worst)
    tlp, tot, cnt = rig.results()
    assert not tlp[[0, 2, 4]].any() and not cnt[[0, 2, 4]].any()  # skipped rows, idle slots: nothing written
    rig2, _ = _run_form(dev, capi, "rows", V, reqs, place, sp, 500)
    assert _by_out_row(rig2, range(6)) == _by_out_row(rig, range(6)), "a second run differs"
    place3 = dict(map=[-1, 2, 4, 1, 6], rows=[3, 1, 2], step=[0, 2, 1], max_new=[8, 8, 8], out_row=[5, 1, 3])
    rig3, scored3 = _run_form(dev, capi, "rows", V, reqs, place3, sp, 600)
    _check(rig3, scored3, "rows, moved", worst)
    assert _by_out_row(rig3, [5, 1, 3]) == _by_out_row(rig, [5, 1, 3]), "a request's results depend on its row, slot or partners"
    # ... and the slots form gives the same bits for the same requests
    place4 = dict(rows=[1, 4, 2], step=[0, 2, 1], max_new=[8, 8, 8], out_row=[5, 1, 3], finished=[])
    rig4, _ = _run_form(dev, capi, "slots", V, reqs, place4, sp, 700)
    assert _by_out_row(rig4, [5, 1, 3]) == _by_out_row(rig, [5, 1, 3]), "the slots and rows forms differ"
    print(f"\n[logprob] rows form V = {V} sample = {do_sample}: worst {worst[0]:.3f} of the bar")
