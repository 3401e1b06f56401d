"""The token sampler (csrc/sampler.hip: sample_kernel in its three modes, sample_slice_kernel) against the float64 reference of
tests/sampler_ref.py, through ops.sample_tokens and ops.sample_logits_slots, in the one-stage form (no workspace) and the
two-stage form (a lent workspace) at every vocabulary size at which the code takes another path:

  V = 512      slices smaller than top_k            V = 128256  the real vocabulary; register sets 0 and 1 of the slices
  V = 1002     V % 4 != 0: the scalar walk; a lent  V = 200000  all four register sets, exact division
               workspace is declined silently       V = 262144  the largest two-stage row
  V = 4100     V / 4 = 1025: a ragged last slice    V = 262148  just past it: one-stage even with a workspace
  misaligned   a logits view one float off a 16-byte boundary (V = 128256): the scalar walk at the real size

What is asserted (sampler_ref's docstring has the rules and where their figures come from): a DECIDED case gives exactly the
reference token, an undecided one a token of its alternatives, at most 2 % of the cases of a test are undecided; the processed
logits have the reference's -inf pattern, finite values within 2^-23 relative, untouched elements bit-equal; every state array
holds exactly what the step should leave; the sentinel bands around every tensor and the workspace's control words are as before.
`pytest -s` prints each test's undecided share and worst processed-logit error; profiles/sampler_bounds.txt records them.
"""
import numpy as np
import pytest
import torch

from tests import sampler_ref as SR

pytestmark = pytest.mark.gpu

GUARD = 16  # elements on either side of every tensor
SENT = -987654321
PAD = 7
_REFS = {}


def _refs(key, scores, hist, hist_len, cap, rep, ngram):
    """The references of every row of an input set under (rep, ngram): computed once, shared by both forms."""
    k = (key, rep, ngram)
    if k not in _REFS:
        _REFS[k] = [SR.Reference(scores[r], SR.clamp_history(hist[r], hist_len[r], cap), rep, ngram) for r in range(scores.shape[0])]
    return _REFS[k]


class Band:
    """A tensor inside a larger sentinel-filled buffer."""

    def __init__(self, init, dev, fill=SENT, shift=0):
        init = torch.as_tensor(init)
        self.n, self.fill = init.numel(), fill
        self.buf = torch.full((self.n + 2 * GUARD + shift,), fill, dtype=init.dtype, device=dev)
        self.lo = GUARD + shift
        self.t = self.buf[self.lo:self.lo + self.n].view(init.shape)
        self.base = init.to(dev)
        self.reset()

    def reset(self):
        self.t.copy_(self.base)

    def check(self, name):
        assert bool((self.buf[:self.lo] == self.fill).all()) and bool((self.buf[self.lo + self.n:] == self.fill).all()), f"write around {name}"

    def np(self):
        return self.t.cpu().numpy()


class Sampler:
    """One input set on the device; call() resets the state, runs one sampler step and returns the state it left."""

    def __init__(self, dev, scores, hist, hist_len, two_stage, out_cap=16, out_rows=None, shift=0):
        from tcavt_amd import capi, ops

        self.capi, self.ops, self.dev = capi, ops, dev
        self.R, self.V = scores.shape
        self.cap, self.out_cap = hist.shape[1], out_cap
        R = self.R
        self.logits = Band(torch.from_numpy(scores), dev, fill=7777.0, shift=shift)  # (shift = 1: one float off the 16-byte boundary)
        self.hist = Band(torch.from_numpy(hist), dev)
        self.hist_len = Band(torch.from_numpy(hist_len.astype(np.int32)), dev)
        self.cur = Band(torch.full((R,), -5, dtype=torch.int64), dev)
        self.pos = Band(torch.arange(R, dtype=torch.int32) + 100, dev)
        self.fin = Band(torch.zeros(R, dtype=torch.int32), dev)
        self.out = Band(torch.full((out_rows or R, out_cap), -1, dtype=torch.int64), dev)
        self.ws = None
        if two_stage:
            nb = int(capi.lib().tcavt_sample_workspace_bytes(R))
            self.ws = Band(torch.zeros(nb, dtype=torch.uint8), dev, fill=0xA5)
        self.bands = {k: getattr(self, k) for k in ("logits", "hist", "hist_len", "cur", "pos", "fin", "out")}

    def two_stage_taken(self):
        return self.ws is not None and self.V % 4 == 0 and self.logits.t.data_ptr() % 16 == 0 and (self.V // 4 + 15) // 16 <= 4096

    def call(self, sp, step, fin=None, slots=None, want_logits=False):
        """step: int (batch form) or int32 array [R] (slots form, slots = (max_new, out_row)).  -> dict of numpy arrays."""
        for b in self.bands.values():
            b.reset()
        if fin is not None:
            self.fin.t.copy_(torch.from_numpy(np.asarray(fin, dtype=np.int32)))
        st = Band(torch.as_tensor(np.atleast_1d(np.asarray(step, dtype=np.int32))), self.dev)
        ws = None if self.ws is None else self.ws.t
        if slots is None:
            self.ops.sample_tokens(self.logits.t, self.hist.t, self.hist_len.t, sp, st.t, self.cur.t, self.pos.t, self.fin.t, self.out.t,
                                   advance_pos=True, workspace=ws)
        else:
            mx, orow = (Band(torch.as_tensor(np.asarray(a, dtype=dt)), self.dev) for a, dt in zip(slots, (np.int32, np.int64)))
            self.ops.sample_logits_slots(self.logits.t, self.hist.t, self.hist_len.t, sp, st.t, mx.t, orow.t, self.cur.t, self.pos.t,
                                         self.fin.t, self.out.t, advance_pos=True, workspace=ws)
        torch.cuda.synchronize()
        for nm, b in self.bands.items():
            b.check(nm)
        st.check("step")
        if slots is not None:
            for b, a, nm in ((mx, slots[0], "max_new"), (orow, slots[1], "out_row")):
                b.check(nm)
                assert np.array_equal(b.np(), np.asarray(a)), f"{nm} changed"
        if self.ws is not None:
            self.ws.check("workspace")
            if self.two_stage_taken():
                assert int(self.ws.t[:64 + 4 * self.R].sum().item()) == 0, "ticket / overflow words not back to zero"
            else:
                assert int(self.ws.t.max().item()) == 0, "a declined workspace was written"
        res = {k: b.np() for k, b in self.bands.items() if k != "logits"}
        res["step"] = st.np()
        if want_logits:
            res["logits"] = self.logits.np()
        return res


def _params(capi, T, k, p, rep, ngram, do_sample, seed, eos=-1):
    return capi.SampleParams(T, p, rep, k, ngram, do_sample, eos, PAD, seed)


def _check_batch_state(s, res, hist0, hl0, step, toks, fin0=None, eos=-1):
    """Everything a batch-form step leaves, given the tokens `toks` the rows chose (finished rows: the pad token)."""
    R, cap, oc = s.R, s.cap, s.out_cap
    fin0 = np.zeros(R, dtype=np.int32) if fin0 is None else np.asarray(fin0)
    emit = np.where(fin0 != 0, PAD, toks)
    out = np.full((R, oc), -1, dtype=np.int64)
    if step < oc:
        out[:, step] = emit
    hist, hl = hist0.copy(), hl0.copy()
    for r in range(R):
        n = min(int(hl0[r]), cap)
        if n < cap:
            hist[r, n] = emit[r]
            hl[r] = n + 1
    assert np.array_equal(res["out"], out), "out_tokens"
    assert np.array_equal(res["cur"], emit), "cur_tok"
    assert np.array_equal(res["hist"], hist), "history"
    assert np.array_equal(res["hist_len"], hl), "hist_len"
    assert np.array_equal(res["pos"], np.arange(R) + 101), "pos"
    assert np.array_equal(res["fin"], ((fin0 != 0) | ((eos >= 0) & (toks == eos))).astype(np.int32)), "finished"
    assert res["step"].tolist() == [step + 1], "step"


def _compare_rows(tally, refs, res_tokens, do_sample, T, k, p, seed, step, rows=None, philox_row=None, label=()):
    for r in (range(len(refs)) if rows is None else rows):
        c = refs[r].choose(do_sample, T, k, p, seed, step if np.isscalar(step) else int(step[r]), r if philox_row is None else int(philox_row[r]))
        tally.token(c, res_tokens[r], label + (r, do_sample, T, k, p, seed))


def _run_sets(s, tally, key, scores, hist, hl, sets, exact_rows=()):
    """sets: (T, k, p, rep, ngram, do_sample, seed, step[, rows]).  One call each; the processed logits are compared the first time a
    (rep, ngram) comes up, the chosen tokens and the state every time."""
    seen = set()
    for st in sets:
        T, k, p, rep, ngram, do_sample, seed, step = st[:8]
        rows = st[8] if len(st) > 8 else None
        refs = _refs(key, scores, hist, hl, s.cap, rep, ngram)
        first = (rep, ngram) not in seen
        seen.add((rep, ngram))
        res = s.call(_params(s.capi, T, k, p, rep, ngram, do_sample, seed), step, want_logits=first)
        toks = res["out"][:, step]
        _compare_rows(tally, refs, toks, do_sample, T, k, p, seed, step, rows=rows, label=(key, rep, ngram))
        _check_batch_state(s, res, hist, hl, step, toks)
        if first:
            for r in range(s.R):
                tally.processed(refs[r], res["logits"][r])


FORMS = pytest.mark.parametrize("two_stage", [False, True], ids=["one-stage", "two-stage"])


@FORMS
@pytest.mark.parametrize("V", [512, 1002, 4100])
def test_full_parameter_grid_at_the_small_vocabularies(gpu, V, two_stage):
    """T {0.7, 1.0, 1.3} x top_k {1, 5, 40, 256} x top_p {0.55, 0.9, 1.0}, two (seed, step) pairs (one seed above 2^32), sampling
    and greedy, the processors cycling through (rep, ngram) = (1.3, 3), (1.0, 0), (1.3, 2), (1.0, 1); then the exact-threshold cases
    (constant and plateau rows, top_k 256, top_p 0.5 / 0.75: the tail lands ON 1 - top_p, and `<=` drops it)."""
    scores, names = SR.rows(V)
    hist, hl = SR.histories(V, scores.shape[0])
    s = Sampler(gpu["device"], scores, hist, hl, two_stage)
    assert s.two_stage_taken() == (two_stage and V % 4 == 0)
    sets = []
    for gi, (T, k, p) in enumerate(SR.GRID):
        rep, ngram = SR.PROCESSORS[gi % len(SR.PROCESSORS)]
        sets += [(T, k, p, rep, ngram, 1, seed, step) for seed, step in SR.SEED_STEPS]
    sets += [(1.0, 1, 1.0, rep, ngram, 0, 0, 2) for rep, ngram in SR.PROCESSORS]
    sets += [(1.0, 256, p, 1.0, 0, 1, seed, step, (2, 5)) for p in (0.5, 0.75) for seed, step in SR.SEED_STEPS]
    tally = SR.Tally(f"grid V={V} {'two' if two_stage else 'one'}-stage")
    _run_sets(s, tally, ("grid", V), scores, hist, hl, sets)
    tally.finish()


LARGE_SETS = (  # (T, k, p, rep, ngram, do_sample, seed, step)
    (0.7, 1, 1.0, 1.3, 3, 1, 1234, 3),
    (1.0, 40, 0.55, 1.0, 0, 1, (1 << 40) + 77, 11),
    (1.3, 256, 1.0, 1.3, 2, 1, 1234, 3),
    (0.9, 40, 0.9, 1.2, 3, 1, 99, 0),
    (1.0, 256, 0.55, 1.3, 3, 1, (1 << 40) + 77, 11),
    (0.7, 5, 0.9, 1.0, 1, 1, 5, 6),
    (1.0, 1, 1.0, 1.3, 3, 0, 0, 2),
    (1.0, 1, 1.0, 1.0, 0, 0, 0, 2),
)


@FORMS
@pytest.mark.parametrize("V", [128256, 200000, 262144, 262148, "misaligned"])
def test_parameter_sets_at_the_large_vocabularies(gpu, V, two_stage):
    shift = 1 if V == "misaligned" else 0
    V = 128256 if shift else V
    scores, names = SR.rows(V)
    assert "100 ties per slice" in names
    hist, hl = SR.histories(V, scores.shape[0])
    s = Sampler(gpu["device"], scores, hist, hl, two_stage, shift=shift)
    assert s.two_stage_taken() == (two_stage and not shift and V <= 262144)
    tally = SR.Tally(f"large V={V}{' misaligned' if shift else ''} {'two' if two_stage else 'one'}-stage")
    _run_sets(s, tally, ("grid", V), scores, hist, hl, LARGE_SETS)
    tally.finish()


HIST_LENS = (0, 1, 2, 3, 4, 5, 511, 512, 513, 1024, 1025, 1500)


def _processor_inputs(V):
    """One row per history length; the histories draw from a small pool -- ids in several slices, 0, V - 1, and five ids out of
    range, two below 0 and two above 2^31 among them -- so that repeats and n-gram matches abound; the pool's scores are the row's
    largest in size, half of them negative: the penalty and the bans decide what is selected."""
    g = np.random.default_rng(4242 + V)
    R, cap = len(HIST_LENS), 1600
    pool = np.array([0, 1, V - 1, V - 2, V // 2, V // 2 + 1, V // 16 + 3, V // 3, (3 * V) // 4, V // 7, 5 * (V // 8) + 2, V - 9,
                     -1, -7, V, (1 << 31) + 5, (1 << 31) + 9], dtype=np.int64)
    scores = (g.standard_normal((R, V)) * 3.0).astype(np.float32)
    ok = pool[(pool >= 0) & (pool < V)]
    scores[:, ok] = (np.where(np.arange(ok.size) % 2 == 0, 1.0, -1.0) * (13.0 + g.random((R, ok.size)))).astype(np.float32)
    hist = pool[g.integers(0, pool.size, size=(R, cap))]
    hl = np.array(HIST_LENS, dtype=np.int32)
    for r in range(R):  # a long history ends on the three ids that also stand at its start: a match for n = 2, 3 and 4 ...
        n = int(hl[r])
        out_a, out_b = ((1 << 31) + 5, (1 << 31) + 9) if r % 2 else (-1, -7)  # (rows 511 / 512: one side of the id range each)
        hist[r, 0:4] = (0, out_a, V // 2 + 1, V // 16 + 3)
        if n >= 8:
            hist[r, n - 3:n] = hist[r, 0:3]
        if n >= 20:  # ... and holds a decoy that differs from them in an out-of-range id only: n = 3 and 4 must not ban V // 5
            hist[r, 10:14] = (0, out_b, V // 2 + 1, V // 5)
    return scores, hist, hl


@FORMS
@pytest.mark.parametrize("V", [512, 128256])
def test_processors_at_every_history_length(gpu, V, two_stage):
    """rep {1.0, 1.3} x ngram {0, 1, 2, 3, 4} on histories of 0, 1, 2 (n = 4: hl + 1 < n, no ban), 3, 4, 5 (the four-wide remainder of
    occurs_before), 511, 512, 513 (the slices' LDS limit), 1024, 1025 (the one-stage form's) and 1500 ids."""
    scores, hist, hl = _processor_inputs(V)
    s = Sampler(gpu["device"], scores, hist, hl, two_stage)
    sets = []
    for rep in (1.0, 1.3):
        for ngram in (0, 1, 2, 3, 4):
            sets.append((0.9, 40, 0.9, rep, ngram, 1, 31 + ngram, 4))
            sets.append((1.0, 1, 1.0, rep, ngram, 0, 0, 4))
    tally = SR.Tally(f"processors V={V} {'two' if two_stage else 'one'}-stage")
    _run_sets(s, tally, ("proc", V), scores, hist, hl, sets)
    refs = _refs(("proc", V), scores, hist, hl, s.cap, 1.0, 4)  # (the inputs do what the docstring says)
    assert not np.isneginf(refs[2].x).any()
    assert all(np.isneginf(refs[r].x[V // 16 + 3]) and np.isfinite(refs[r].x[V // 5]) for r in range(6, len(HIST_LENS)))
    tally.finish()


@FORMS
def test_bookkeeping_edges_of_the_batch_form(gpu, two_stage):
    """hist_len == hist_cap (nothing appended, the length unchanged), hist_len > hist_cap (clamped), a finished row (emits the pad
    token, its selection stays out of the output), a row that draws EOS, step >= out_cap (no output write, the state advances)."""
    V, cap = 512, 40
    scores, _ = SR.rows(V, extra=False)
    scores = scores[[0, 1, 5, 6, 7, 0]]
    hist, _ = SR.histories(V, 6, cap)
    hist[:, 30:] = hist[:, :10]
    hl = np.array([cap, cap + 5, 30, 30, 12, 0], dtype=np.int32)
    fin0 = np.array([0, 0, 1, 0, 0, 0], dtype=np.int32)
    s = Sampler(gpu["device"], scores, hist, hl, two_stage, out_cap=4)
    tally = SR.Tally(f"bookkeeping {'two' if two_stage else 'one'}-stage")
    T, k, p, rep, ngram, seed = 0.9, 40, 0.9, 1.3, 3, 21
    refs = _refs(("book", V), scores, hist, hl, cap, rep, ngram)
    for step in (2, 4, 9):
        eos = refs[4].choose(1, T, k, p, seed, step, 4).token
        res = s.call(_params(s.capi, T, k, p, rep, ngram, 1, seed, eos=eos), step, fin=fin0, want_logits=True)
        hist_after = res["hist"]
        toks = np.array([hist_after[r, min(int(hl[r]), cap)] if min(int(hl[r]), cap) < cap else res["cur"][r] for r in range(6)])
        live = [r for r in range(6) if not fin0[r]]
        _compare_rows(tally, refs, toks, 1, T, k, p, seed, step, rows=live, label=("book", step))
        chosen = np.array([PAD if fin0[r] else toks[r] for r in range(6)])
        _check_batch_state(s, res, hist, hl, step, chosen, fin0=fin0, eos=eos)
        assert res["fin"][4] == 1 or not refs[4].choose(1, T, k, p, seed, step, 4).decided
        for r in range(6):  # the processors run on finished rows too, on the clamped history
            tally.processed(refs[r], res["logits"][r])
    tally.finish()


@FORMS
@pytest.mark.parametrize("V", [512, 128256])
def test_slots_form_with_mixed_steps(gpu, V, two_stage):
    """ops.sample_logits_slots: every slot at its own step, out_row (a permutation into more requests than slots) is both the output
    row and the Philox row; a finished slot is inert but for cur_tok = pad; a slot ends at its budget; step >= out_cap writes nothing."""
    scores, _ = SR.rows(V, extra=False)
    S, oc = scores.shape[0], 8
    hist, hl = SR.histories(V, S)
    step = np.array([0, 3, 1, 7, 2, 5, 9, 4], dtype=np.int32)
    orow = np.array([9, 2, 7, 0, 5, 3, 8, 1], dtype=np.int64)
    mx = np.array([20, 4, 20, 20, 3, 20, 20, 20], dtype=np.int32)  # slots 1 and 4 reach their budget with this token
    fin0 = np.array([0, 0, 1, 0, 0, 0, 0, 0], dtype=np.int32)
    s = Sampler(gpu["device"], scores, hist, hl, two_stage, out_cap=oc, out_rows=10)
    tally = SR.Tally(f"slots V={V} {'two' if two_stage else 'one'}-stage")
    sets = SR.GRID[::2] + SR.GRID[1::2][::-1]  # (the reduced grid: every other point under one seed, the rest under the other)
    for gi, (T, k, p) in enumerate(sets + [(None, 1, 1.0)]):  # (the last one: greedy)
        rep, ngram = SR.PROCESSORS[gi % len(SR.PROCESSORS)]
        do_sample = 0 if T is None else 1
        T, k, p = (1.0, 1, 1.0) if not do_sample else (T, k, p)
        seed = (1 << 40) + 77 if gi >= len(SR.GRID) // 2 else 1234
        refs = _refs(("slots", V), scores, hist, hl, s.cap, rep, ngram)
        res = s.call(_params(s.capi, T, k, p, rep, ngram, do_sample, seed), step, fin=fin0, slots=(mx, orow))
        live = [r for r in range(S) if not fin0[r]]
        toks = np.array([res["hist"][r, 30] for r in range(S)])  # (every history holds 30 ids of 40: the token is appended)
        _compare_rows(tally, refs, toks, do_sample, T, k, p, seed, step, rows=live, philox_row=orow, label=("slots", V, gi))
        out = np.full((10, oc), -1, dtype=np.int64)
        h2, l2, st2, fin2 = hist.copy(), hl.copy(), step.copy(), fin0.copy()
        cur, pos = np.full(S, -5, dtype=np.int64), np.arange(S) + 100
        for r in range(S):
            if fin0[r]:
                cur[r] = PAD
                continue
            if step[r] < oc:
                out[orow[r], step[r]] = toks[r]
            cur[r], h2[r, 30], l2[r], pos[r], st2[r] = toks[r], toks[r], 31, pos[r] + 1, step[r] + 1
            fin2[r] = int(step[r] + 1 == mx[r])
        for nm, want in (("out", out), ("cur", cur), ("hist", h2), ("hist_len", l2), ("pos", pos), ("fin", fin2), ("step", st2)):
            assert np.array_equal(res[nm], want), (nm, gi)
    tally.finish()
