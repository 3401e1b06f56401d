"""The chain tcavt_constraint_mask -> tcavt_sample_tokens -> tcavt_constraint_advance over six steps of the batch form, on the
logits rows of sampler_ref.rows(V), against sampler_ref.Reference run on host-masked rows (tests/constraint_ref.py): greedy rows
and sampled rows over a small part of sampler_ref.GRID with no_repeat = 0, in the one-stage form and in the workspace (two-stage)
form.  sampler_ref's decision rule and its UNDECIDED_CAP hold unchanged; tests/test_constraint_cpu.py checks that the reference
alone stays under the cap on these allowed sets.  A constraint that allows everything gives the tokens of the call without the
bracket, bit for bit."""
import numpy as np
import pytest
import torch

from tests import constraint_ref as CR
from tests import sampler_ref as SR

pytestmark = pytest.mark.gpu

V, CAP, PAD = CR.V, CR.CAP, 7
_inputs = CR.sampler_inputs


class Device:
    def __init__(self, dev, scores, hist, hl, two_stage):
        from tcavt_amd import capi, ops

        self.ops, self.capi, R = ops, capi, scores.shape[0]
        self.base = torch.from_numpy(scores).to(dev)
        self.logits = self.base.clone()
        self.hist, self.hl = torch.from_numpy(hist).to(dev), torch.from_numpy(hl.astype(np.int32)).to(dev)
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.cur, self.pos = torch.zeros(R, dtype=torch.int64, device=dev), torch.zeros(R, dtype=torch.int32, device=dev)
        self.fin = torch.zeros(R, dtype=torch.int32, device=dev)
        self.out = torch.full((R, CR.STEPS), -1, dtype=torch.int64, device=dev)
        self.ws = ops.sample_workspace(R, dev) if two_stage else None

    def sample(self, sp):
        self.ops.sample_tokens(self.logits, self.hist, self.hl, sp, self.step, self.cur, self.pos, self.fin, self.out, advance_pos=True,
                               workspace=self.ws)


@pytest.mark.parametrize("two_stage", [False, True], ids=["one-stage", "two-stage"])
def test_constrained_selection_matches_the_reference_on_masked_rows(gpu, two_stage):
    from tcavt_amd import ops

    dev = gpu["device"]
    scores, hist, hl = _inputs()
    R = scores.shape[0]
    C = CR.cycle_constraint(V)
    T = ops.ConstraintTable(C.token_class, C.trans, dev).build()
    starts = np.arange(R, dtype=np.int32) % 3
    tally = SR.Tally(f"constraint chain, {'two' if two_stage else 'one'}-stage")
    for params in CR.SETS:
        temp, k, p, rep, do_sample, seed = params
        d = Device(dev, scores, hist, hl, two_stage)
        sp = d.capi.SampleParams(temp, p, rep, k, 0, do_sample, -1, PAD, seed)
        state = torch.full((R,), 2, dtype=torch.int32, device=dev)  # stale words: step 0 takes the start states
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        cws = torch.empty(ops.constraint_workspace_bytes(R), dtype=torch.uint8, device=dev)
        a = ops.constraint_args(T, d.logits, d.step, d.fin, d.cur, state, torch.from_numpy(starts).to(dev), cws, flag=flag)
        chain = CR.Chain(C, scores, hist, hl, CAP, params, starts, tally)
        for t in range(CR.STEPS):
            d.logits.copy_(d.base)
            ops.constraint_mask(a)
            d.sample(sp)
            ops.constraint_advance(a)
            torch.cuda.synchronize()
            got = d.out[:, t].cpu().numpy()
            assert np.array_equal(got, d.cur.cpu().numpy())
            chain.step(t, got)  # (asserts that every token is allowed where the reference stands)
            assert state.cpu().tolist() == chain.state and flag.item() == 0, (params, t)
        assert d.step.item() == CR.STEPS
    tally.finish()


@pytest.mark.parametrize("two_stage", [False, True], ids=["one-stage", "two-stage"])
def test_a_free_constraint_gives_the_tokens_of_the_call_without_the_bracket(gpu, two_stage):
    from tcavt_amd import ops
    from tcavt_amd.constraint import TokenConstraint

    dev = gpu["device"]
    scores, hist, hl = _inputs()
    R = scores.shape[0]
    C = TokenConstraint.free(V)
    T = ops.ConstraintTable(C.token_class, C.trans, dev).build()
    for temp, k, p, rep, do_sample, seed in CR.SETS:
        outs = []
        for bracket in (False, True):
            d = Device(dev, scores, hist, hl, two_stage)
            sp = d.capi.SampleParams(temp, p, rep, k, 0, do_sample, -1, PAD, seed)
            state = torch.zeros(R, dtype=torch.int32, device=dev)
            cws = torch.empty(ops.constraint_workspace_bytes(R), dtype=torch.uint8, device=dev)
            a = ops.constraint_args(T, d.logits, d.step, d.fin, d.cur, state, torch.zeros(R, dtype=torch.int32, device=dev), cws)
            for t in range(CR.STEPS):
                d.logits.copy_(d.base)
                if bracket:
                    ops.constraint_mask(a)
                d.sample(sp)
                if bracket:
                    ops.constraint_advance(a)
            torch.cuda.synchronize()
            outs.append((d.out.cpu(), d.logits.cpu(), d.hist.cpu()))
        for x, y in zip(*outs):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
