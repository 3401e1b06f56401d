"""tcavt_beam_select + tcavt_beam_reorder, driven step by step on synthetic fp32 logits against the float64 reference of
tests/beam_ref.py.  At every step the reference starts from the device's own fp32 state, so errors do not accumulate:

  select   candidate sets, parents, tokens, live flags, the finished store and the unsat / done / finished flags must be EQUAL to
           the reference's; acc within pen * (1e-5 + 2^-22 |ref lp|) + 2^-23 |acc| (the bar of tests/logprob_ref.py scaled by the
           penalty, plus one rounding of the sum); finished scores bit-equal to float32(acc) / len_pow[s].  Precondition, asserted:
           the reference's smallest decision margin -- the gaps inside the top K + 1 and between finished scores -- is >= 4 bars,
           so a bad seed fails loudly instead of hiding a difference.  The seeds below were picked on the CPU (simulate()).
  reorder  history and suffix rows of beam j are those of its parent, bit for bit; slots beyond the written ones, done prompts
           and the guard bands around every buffer are untouched; hist_len, pos and step advance.

Rows are 3 * N(0, 1) seeded from (seed, prompt, generated prefix), with the EOS id lifted above the row maximum in about a third of
the rows.  B = 2 prompts with ragged prompt lengths.  `pytest -s` prints the worst acc error in units of the bar per case."""
import numpy as np
import pytest
import torch

import beam_ref as BR

pytestmark = pytest.mark.gpu

GUARD, SENT = 64, -77
PAD, NQ, LAYERS, NKV = 3, 2, 2, 1
ABS, REL = 1e-5, 2.0 ** -22
PROMPT_LENS = (5, 3)
# (V, n, N) -> seed; simulate() gives margins of 399, 231, 18, 60 and 32 bars (a bar is about 2e-5) and hypotheses of 1 .. N tokens
SHAPES = {(48, 2, 6): 2, (1003, 4, 6): 1, (1003, 16, 5): 6, (128256, 8, 6): 7, (128256, 16, 4): 5}
SMALL = {(48, 2, 6): 6, (1003, 4, 6): 1}  # penalty 1.0, length_penalty 0.5, early_stopping=True: 1737 and 275 bars


def row_fn(seed, V, eos):
    def fn(b, prefix):
        g = np.random.default_rng([seed, b, len(prefix), *[int(t) for t in prefix]])
        x = (3.0 * g.standard_normal(V)).astype(np.float32)
        if g.random() < 1 / 3:
            x[eos] = x.max() + np.float32(0.5)
        return x
    return fn


def prompts(V, seed):
    g = np.random.default_rng(seed + 99)
    return [g.integers(0, V, size=L).tolist() for L in PROMPT_LENS]


def bar(pen, lp_ref, acc_ref):
    return pen * (ABS + REL * abs(lp_ref)) + 2.0 ** -23 * abs(acc_ref)


def reference_step(row_of, prompt, state, n, pen, ng):
    """The reference's candidates from ``state`` (K + 1 of them, for the margin) and their processed log-probabilities;
    row_of(j) -> the raw row of beam j."""
    rows = [BR.processed(row_of(j), prompt + state.tokens[j], pen, ng) if state.live[j] else None for j in range(n)]
    cands = BR.candidates(rows, state.run_score, state.live, n, k=2 * n + 1)
    return cands, [float(rows[p][t]) for p, t, _ in cands]


def margin_in_bars(cands, lps, pen):
    """Smallest gap between neighbours of the top K + 1, in units of the larger of the two bars."""
    worst = np.inf
    for (_, _, a0), (_, _, a1), l0, l1 in zip(cands[:-1], cands[1:], lps[:-1], lps[1:]):
        if np.isfinite(a1):
            worst = min(worst, (a0 - a1) / max(bar(pen, l0, a0), bar(pen, l1, a1)))
    return worst


def simulate(V, n, N, seed, pen=1.2, ng=3, lpen=1.0, early=False):
    """CPU only: the search of both prompts by the reference alone -> (smallest margin in bars, hypothesis lengths).  How the seeds
    above were chosen: margin >= 4 bars with room to spare and hypotheses of different lengths."""
    eos, fn, worst, lens = V // 3, row_fn(seed, V, V // 3), np.inf, []
    lpow = BR.len_pow_table(N, lpen, np.float32)
    for b, prompt in enumerate(prompts(V, seed)):
        st = BR.State(n)
        for s in range(N):
            cands, lps = reference_step(lambda j: fn(b, st.tokens[j]), prompt, st, n, pen, ng)
            worst = min(worst, margin_in_bars(cands, lps, pen))
            step_bar = max(bar(pen, l, a) for (_, _, a), l in zip(cands, lps) if np.isfinite(a))
            c32 = [(p, t, float(np.float32(a))) for p, t, a in cands[:2 * n]]
            BR.advance(st, c32, s, N, eos, lpow[s], early, div=lambda a, l: float(np.float32(a) / np.float32(l)), pad=PAD)
            fs = sorted(sc for _, sc in st.fin)
            for x0, x1 in zip(fs[:-1], fs[1:]):
                worst = min(worst, (x1 - x0) * float(lpow[s]) / step_bar) if x1 > x0 else worst
            if st.done:
                break
        lens += [len(t) for t, _ in st.fin]
    return worst, lens


class Band:
    """A tensor inside a larger sentinel-filled buffer."""

    def __init__(self, init, dev):
        init = torch.as_tensor(init)
        self.n, self.fill = init.numel(), (179 if init.dtype == torch.uint8 else SENT)
        self.buf = torch.full((self.n + 2 * GUARD,), self.fill, dtype=init.dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + self.n].view(init.shape)
        self.t.copy_(init)

    def check(self, name):
        assert bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all()), f"write around {name}"

    def np(self):
        return self.t.cpu().numpy()


class Rig:
    """The device state of a beam search on B prompts x n beams, every array between guard bands, and the two argument structs."""

    def __init__(self, dev, V, n, N, prompt_lists, pen, ng, lpen, early, eos, trace=True):
        from tcavt_amd import ops

        self.ops, self.dev = ops, dev
        self.V, self.n, self.N, self.B = V, n, N, len(prompt_lists)
        self.pen, self.ng, self.early, self.eos = pen, ng, early, eos
        self.prompts = prompt_lists
        B, R = self.B, self.B * n
        self.R, self.cap, self.lmax = R, max(len(p) for p in prompt_lists) + N, max(N - 1, 1)
        i32, i64, f32 = torch.int32, torch.int64, torch.float32
        hist = torch.full((R, self.cap), 1, dtype=i64)
        plen = torch.tensor([len(p) for p in prompt_lists], dtype=i32)
        for b, p in enumerate(prompt_lists):
            hist[b * n:(b + 1) * n, :len(p)] = torch.tensor(p, dtype=i64)
        live = torch.zeros(B, n, dtype=i32)
        live[:, 0] = 1
        self.lpow = BR.len_pow_table(N, lpen, np.float32)
        mk = lambda init: Band(init, dev)  # noqa: E731
        self.logits = mk(torch.zeros(R, V, dtype=f32))
        self.history, self.hist_len = mk(hist), mk(plen.repeat_interleave(n))
        self.run_score, self.live = mk(torch.zeros(R, dtype=f32)), mk(live)
        self.fin_tokens = mk(torch.full((B, n, N), SENT, dtype=i64))
        self.fin_score, self.fin_flag, self.fin_len = mk(torch.zeros(B, n, dtype=f32)), mk(torch.zeros(B, n, dtype=i32)), mk(torch.zeros(B, n, dtype=i32))
        self.unsat, self.done = mk(torch.ones(B, dtype=i32)), mk(torch.zeros(B, dtype=i32))
        self.cur, self.pos, self.finished = mk(torch.zeros(R, dtype=i64)), mk((plen + NQ).repeat_interleave(n)), mk(torch.zeros(R, dtype=i32))
        self.step, self.prefix_len = mk(torch.zeros(B, dtype=i32)), mk(plen + NQ)
        self.len_pow = mk(torch.from_numpy(self.lpow))
        self.parent, self.plan = mk(torch.full((R,), SENT, dtype=i32)), mk(torch.full((B, 4), SENT, dtype=i32))
        self.trace = mk(torch.full((N, B, 2 * n, 3), SENT, dtype=i32)) if trace else None
        self.ws = mk(torch.randint(0, 255, (ops.beam_workspace_bytes(R),), dtype=torch.uint8))  # starts as garbage
        g = torch.Generator().manual_seed(5)
        self.sk = mk(torch.randn(LAYERS, R, self.lmax, NKV * 64, generator=g).to(torch.float16))
        self.sv = mk(torch.randn(LAYERS, R, self.lmax, NKV * 64, generator=g).to(torch.float16))
        self.sel = ops.beam_args(self.logits.t, n, N, self.history.t, self.hist_len.t, self.run_score.t, self.live.t, self.fin_tokens.t,
                                 self.fin_score.t, self.fin_flag.t, self.fin_len.t, self.unsat.t, self.done.t, self.cur.t, self.pos.t,
                                 self.finished.t, self.step.t, self.prefix_len.t, self.len_pow.t, self.parent.t, self.plan.t, self.ws.t,
                                 eos, PAD, pen, ng, early, trace=self.trace.t if trace else None)
        self.reo = ops.beam_reorder_args(n, self.parent.t, self.plan.t, self.cur.t, self.history.t, self.hist_len.t, self.pos.t,
                                         self.step.t, self.sk.t, self.sv.t, LAYERS, NKV)
        self.worst = 0.0

    BANDS = ("logits", "history", "hist_len", "run_score", "live", "fin_tokens", "fin_score", "fin_flag", "fin_len", "unsat", "done",
             "cur", "pos", "finished", "step", "prefix_len", "len_pow", "parent", "plan", "ws", "sk", "sv")
    STATE = ("history", "hist_len", "run_score", "live", "fin_tokens", "fin_score", "fin_flag", "fin_len", "unsat", "done", "cur", "pos",
             "finished", "step", "sk", "sv")

    def check_bands(self):
        for nm in self.BANDS + (("trace",) if self.trace is not None else ()):
            getattr(self, nm).check(nm)

    def snapshot(self):
        """The state as numpy copies."""
        return {nm: np.array(getattr(self, nm).np(), copy=True) for nm in self.STATE}

    def host_state(self, b, snap):
        """The reference's State of prompt b from the device's arrays."""
        n, L = self.n, len(self.prompts[b])
        s = int(snap["step"][b])
        st = BR.State(n)
        st.tokens = [snap["history"][b * n + j, L:L + s].tolist() for j in range(n)]
        st.run_score = [float(x) for x in snap["run_score"][b * n:(b + 1) * n]]
        st.live = [bool(x) for x in snap["live"][b]]
        st.fin = [(snap["fin_tokens"][b, i, :snap["fin_len"][b, i]].tolist(), float(snap["fin_score"][b, i]))
                  for i in range(n) if snap["fin_flag"][b, i]]
        st.unsat, st.done = bool(snap["unsat"][b]), bool(snap["done"][b])
        return st

    def step_once(self, fn, check_margin=True):
        """One decode-write + select + reorder with every check; fn(b, generated tokens) -> the raw row."""
        n, N, V, B = self.n, self.N, self.V, self.B
        before = self.snapshot()
        steps = before["step"]
        # what the decode step would have done: the rows' keys / values of the slot just written (distinct per row and step)
        for b in range(B):
            s = int(steps[b])
            if s > 0 and not before["done"][b]:
                g = torch.Generator().manual_seed(1000 * s + b)
                for c in (self.sk, self.sv):
                    c.t[:, b * n:(b + 1) * n, s - 1] = torch.randn(LAYERS, n, NKV * 64, generator=g).to(torch.float16).to(self.dev)
        before = self.snapshot()
        states = [self.host_state(b, before) for b in range(B)]
        x = np.zeros((self.R, V), dtype=np.float32)
        for b in range(B):
            for j in range(n):
                if states[b].live[j] and not states[b].done:
                    x[b * n + j] = fn(b, states[b].tokens[j])
        self.logits.t.copy_(torch.from_numpy(x))
        self.ops.beam_select(self.sel)
        torch.cuda.synchronize()
        self.check_bands()
        assert np.array_equal(self.logits.np(), x), "logits were written"
        mid = self.snapshot()
        parent, plan = self.parent.np(), self.plan.np()
        trace = self.trace.np() if self.trace is not None else None
        for b in range(B):
            st, s, L = states[b], int(steps[b]), len(self.prompts[b])
            rows = slice(b * n, (b + 1) * n)
            if st.done or s >= N:  # inert: nothing of the prompt moves
                assert plan[b, 0] == -1 and parent[rows].tolist() == list(range(n))
                for nm in self.STATE:
                    assert np.array_equal(_share(mid, nm, b, n), _share(before, nm, b, n)), (nm, b)
                continue
            cands, lps = reference_step(lambda j: x[b * n + j], self.prompts[b], st, n, self.pen, self.ng)
            step_bar = max(bar(self.pen, l, a) for (_, _, a), l in zip(cands, lps) if np.isfinite(a))
            if check_margin:
                assert margin_in_bars(cands, lps, self.pen) >= 4.0, ("decision margin below 4 bars: pick another seed", b, s)
            K = 2 * n
            got = [(int(trace[s, b, k, 0]), int(trace[s, b, k, 1]), float(trace[s, b, k, 2:3].view(np.float32)[0])) for k in range(K)]
            assert [(p, t) for p, t, _ in got] == [(p, t) for p, t, _ in cands[:K]], (b, s)
            for (_, _, a), (_, _, ar), lr in zip(got, cands[:K], lps[:K]):
                if np.isfinite(ar):
                    self.worst = max(self.worst, abs(a - ar) / bar(self.pen, lr, ar))
                    assert abs(a - ar) <= bar(self.pen, lr, ar), (b, s, a, ar)
                else:
                    assert a == ar
            # steps 3 to 7 from the device's own acc values, with the device's division
            info = BR.advance(st, got, s, N, self.eos, self.lpow[s], self.early, pad=PAD,
                              div=lambda a, l: float(np.float32(a) / np.float32(l)))
            if check_margin and len(st.fin) > 1:
                fs = sorted(sc for _, sc in st.fin)
                gaps = [x1 - x0 for x0, x1 in zip(fs[:-1], fs[1:]) if x1 > x0]
                assert not gaps or min(gaps) * float(self.lpow[s]) >= 4.0 * step_bar, ("finished scores too close", b, s)
            assert parent[rows].tolist() == info["parent"], (b, s)
            assert mid["cur"][rows].tolist() == info["token"], (b, s)
            assert mid["live"][b].tolist() == [int(v) for v in st.live]
            for j in range(n):
                if st.live[j]:
                    assert np.float32(mid["run_score"][b * n + j]) == np.float32(st.run_score[j])
            assert mid["fin_flag"][b].tolist() == [1] * len(st.fin) + [0] * (n - len(st.fin)), (b, s)
            for i, (toks, sc) in enumerate(st.fin):
                assert mid["fin_len"][b, i] == len(toks)
                assert mid["fin_tokens"][b, i].tolist() == toks + [PAD] * (N - len(toks)), (b, s, i)
                assert np.float32(mid["fin_score"][b, i]).tobytes() == np.float32(sc).tobytes(), (b, s, i)
            assert bool(mid["unsat"][b]) == st.unsat and bool(mid["done"][b]) == st.done, (b, s)
            assert mid["finished"][rows].tolist() == [int(st.done)] * n
            t_slots = int(before["pos"][b * n]) - int(self.prefix_len.np()[b]) + 1 if s > 0 else 0
            assert plan[b].tolist() == [s, t_slots, int(info["parent"] != list(range(n))), L], (b, s, plan[b])
            for nm in ("history", "hist_len", "pos", "step", "sk", "sv"):  # the selection leaves these to the reorder
                assert np.array_equal(_share(mid, nm, b, n), _share(before, nm, b, n)), nm
        # ---- reorder
        self.ops.beam_reorder(self.reo)
        torch.cuda.synchronize()
        self.check_bands()
        after = self.snapshot()
        for b in range(B):
            s, L, rows = int(steps[b]), len(self.prompts[b]), slice(b * n, (b + 1) * n)
            if plan[b, 0] < 0:
                for nm in self.STATE:
                    assert np.array_equal(_share(after, nm, b, n), _share(before, nm, b, n)), (nm, b)
                continue
            par = parent[rows]
            want_h = mid["history"][rows].copy()
            want_h[:, L:L + s] = mid["history"][rows][par, L:L + s]
            want_h[:, L + s] = mid["cur"][rows]
            assert np.array_equal(after["history"][rows], want_h), (b, s)
            assert after["hist_len"][rows].tolist() == [L + s + 1] * n and after["step"][b] == s + 1
            assert np.array_equal(after["pos"][rows], mid["pos"][rows] + (1 if s > 0 else 0))
            for nm in ("sk", "sv"):
                want = mid[nm][:, rows].copy()
                want[:, :, :s] = mid[nm][:, rows][:, par, :s]  # slots 0 .. s - 1 follow the parents; the rest stays
                assert np.array_equal(after[nm][:, rows].view(np.uint16), want.view(np.uint16)), (nm, b, s)
            for nm in ("run_score", "live", "fin_tokens", "fin_score", "fin_flag", "fin_len", "unsat", "done", "cur", "finished"):
                assert np.array_equal(_share(after, nm, b, n), _share(mid, nm, b, n)), nm
        return after


def _share(snap, nm, b, n):
    a = snap[nm]
    if nm in ("sk", "sv"):
        return a[:, b * n:(b + 1) * n]
    if nm in ("live", "fin_tokens", "fin_score", "fin_flag", "fin_len", "unsat", "done", "step"):
        return a[b]
    return a[b * n:(b + 1) * n]


def run_search(rig, fn, steps=None, check_margin=True):
    out = None
    for _ in range(rig.N if steps is None else steps):
        out = rig.step_once(fn, check_margin)
    return out


@pytest.mark.parametrize("shape", list(SHAPES))
def test_search_matches_reference_step_by_step(gpu, shape):
    V, n, N = shape
    seed, eos = SHAPES[shape], V // 3
    rig = Rig(gpu["device"], V, n, N, prompts(V, seed), 1.2, 3, 1.0, False, eos)
    end = run_search(rig, row_fn(seed, V, eos))
    assert end["fin_flag"].all() and end["done"].all()
    lens = end["fin_len"].reshape(-1)
    assert lens.min() >= 1 and lens.max() <= N
    print(f"\n{shape}: worst acc error {rig.worst:.3f} bars, hypothesis lengths {sorted(lens.tolist())}")


@pytest.mark.parametrize("shape", list(SMALL))
def test_search_without_penalty_with_length_penalty_and_early_stopping(gpu, shape):
    V, n, N = shape
    seed, eos = SMALL[shape], V // 3
    rig = Rig(gpu["device"], V, n, N, prompts(V, seed), 1.0, 3, 0.5, True, eos)
    end = run_search(rig, row_fn(seed, V, eos))
    assert end["done"].all()
    print(f"\n{shape}: worst acc error {rig.worst:.3f} bars, hypothesis lengths {sorted(end['fin_len'].reshape(-1).tolist())}")


def test_two_launches_and_a_prompt_alone_give_the_same_bits(gpu):
    """The whole search twice -> the same bits; prompt 1 alone (B = 1) -> the bits it has beside prompt 0."""
    V, n, N = 1003, 4, 6
    seed, eos = SHAPES[(V, n, N)], V // 3
    ps, fn = prompts(V, seed), row_fn(seed, V, eos)
    ends = []
    for _ in range(2):
        rig = Rig(gpu["device"], V, n, N, ps, 1.2, 3, 1.0, False, eos)
        ends.append((run_search(rig, fn), rig.trace.np().copy()))
    for nm in Rig.STATE:
        assert np.array_equal(ends[0][0][nm], ends[1][0][nm]), nm
    assert np.array_equal(ends[0][1], ends[1][1])
    alone = Rig(gpu["device"], V, n, N, ps[1:], 1.2, 3, 1.0, False, eos)
    end = run_search(alone, lambda b, pre: fn(1, pre))
    for nm in ("run_score", "fin_tokens", "fin_score", "fin_flag", "fin_len", "unsat", "done", "cur"):
        assert np.array_equal(_share(end, nm, 0, n), _share(ends[0][0], nm, 1, n)), nm
    assert np.array_equal(alone.trace.np()[:, 0], ends[0][1][:, 1])


def _planted_rig(dev, n, N, s, gen_tokens, V=48, ng=3):
    """A hand-made state at step s: one prompt [7, 8, 9], beam j holds gen_tokens[j], every beam live with run_score -j."""
    rig = Rig(dev, V, n, N, [[7, 8, 9]], 1.0, ng, 1.0, False, -1)
    h = rig.history.np().copy()
    for j, toks in enumerate(gen_tokens):
        h[j, 3:3 + s] = toks
    rig.history.t.copy_(torch.from_numpy(h))
    rig.hist_len.t.fill_(3 + s)
    rig.pos.t.fill_(3 + NQ + s - 1)
    rig.step.t.fill_(s)
    rig.live.t.fill_(1)
    rig.run_score.t.copy_(torch.arange(n, dtype=torch.float32) * -1.0)
    return rig


def test_planted_ban_follows_the_parents_history(gpu):
    """Both new beams come from beam 1, whose tokens end in 20 21 22 20; after the reorder row 0 holds ... 20 21 22 20 21, so the
    next selection must ban 22 on row 0 -- with row 0's old history (1 2 3 4) it would not."""
    rig = _planted_rig(gpu["device"], 2, 8, 4, [[1, 2, 3, 4], [20, 21, 22, 20]])

    def rows_a(b, pre):
        x = np.full(48, -5.0, dtype=np.float32)
        if list(pre) == [20, 21, 22, 20]:
            x[21], x[5] = 9.0, 8.0
        return x

    rig.step_once(rows_a, check_margin=False)
    assert rig.parent.np().tolist() == [1, 1]  # all beams from one parent
    assert rig.history.np()[0, 3:8].tolist() == [20, 21, 22, 20, 21] and rig.history.np()[1, 3:8].tolist() == [20, 21, 22, 20, 5]

    def rows_b(b, pre):
        x = np.linspace(-4.0, -3.0, 48).astype(np.float32)
        x[22] = 9.0
        return x

    rig.step_once(rows_b, check_margin=False)
    tr = rig.trace.np()[5, 0]
    assert (0, 22) not in [(int(p), int(t)) for p, t, _ in tr] and (1, 22) in [(int(p), int(t)) for p, t, _ in tr]


@pytest.mark.parametrize("name,n,par", [("swap", 2, [1, 0]), ("one parent", 4, [2, 2, 2, 2]), ("identity", 4, [0, 1, 2, 3]),
                                        ("rotation of 16", 16, [(j + 5) % 16 for j in range(16)])])
def test_planted_reorder(gpu, name, n, par):
    """tcavt_beam_reorder on a hand-made plan: rows follow `par` in slots 0 .. 2 and in the generated part of the history; slot 3
    on, the prompt part and everything around the buffers stay; a second prompt that is done (plan -1) is not touched."""
    dev, N, s = gpu["device"], 8, 3
    rig = Rig(dev, 48, n, N, [[7, 8, 9], [4, 5]], 1.0, 0, 1.0, False, -1)
    g = torch.Generator().manual_seed(11)
    rig.history.t.copy_(torch.randint(0, 48, rig.history.t.shape, generator=g).to(dev))
    rig.hist_len.t.copy_(torch.tensor([3 + s] * n + [2 + s] * n, dtype=torch.int32))
    rig.cur.t.copy_(torch.arange(100, 100 + 2 * n))
    rig.step.t.fill_(s)
    rig.parent.t.copy_(torch.tensor(par + par, dtype=torch.int32))
    rig.plan.t.copy_(torch.tensor([[s, s, int(par != list(range(n))), 3], [-1, s, 1, 2]], dtype=torch.int32))
    before = rig.snapshot()
    rig.ops.beam_reorder(rig.reo)
    torch.cuda.synchronize()
    rig.check_bands()
    after = rig.snapshot()
    for nm in rig.STATE:  # prompt 1: done
        assert np.array_equal(_share(after, nm, 1, n), _share(before, nm, 1, n)), nm
    want = before["history"][:n].copy()
    want[:, 3:3 + s] = before["history"][:n][par, 3:3 + s]
    want[:, 3 + s] = np.arange(100, 100 + n)
    assert np.array_equal(after["history"][:n], want)
    assert after["hist_len"][:n].tolist() == [4 + s] * n and after["step"][0] == s + 1
    assert np.array_equal(after["pos"][:n], before["pos"][:n] + 1)
    for nm in ("sk", "sv"):
        w = before[nm][:, :n].copy()
        w[:, :, :s] = before[nm][:, :n][:, par, :s]
        assert np.array_equal(after[nm][:, :n].view(np.uint16), w.view(np.uint16)), nm
