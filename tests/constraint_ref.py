"""Host reference of constrained decoding -- TEST INFRASTRUCTURE ONLY, numpy only: mask a logits row by
``TokenConstraint.allowed(state)``, then the processors and the selection of tests/sampler_ref.py.  HF's order is penalty, bans,
PrefixConstrainedLogitsProcessor, warpers; the penalty and the warpers never turn -inf into a finite score, so masking first gives
the same row.

``greedy`` is what tests/test_constraint_reference_cpu.py replays HF's sequences with; ``cycle_constraint`` and ``Chain`` are the
automaton and the step-by-step reference that the sampler tests (CPU and GPU) share."""
import numpy as np
import torch

from tests import sampler_ref as SR


def masked(C, state, scores):
    """scores fp32 [V] with -inf over the ids ``state`` does not allow."""
    x = np.array(scores, dtype=np.float32, copy=True)
    ok = np.zeros(x.size, dtype=bool)
    ok[C.allowed(state)] = True
    x[~ok] = -np.inf
    return x


def greedy(C, state, scores, hist, repetition_penalty=1.0):
    """The arg-max (first maximum) of the masked, processed row."""
    x, _ = SR.process_logits(masked(C, state, scores), hist, repetition_penalty, 0)
    return int(np.argmax(x))


def cycle_constraint(V):
    """Three states in a cycle, each allowing another part of the vocabulary -- ids with id % 3 == 0, with id % 3 == 1, with
    id % 5 == 0 -- plus, in every state, the few ids at which the sparse rows of sampler_ref.rows are finite (5, V // 2, V - 3,
    V - 1) and the 300 ids of its plateau row (a plateau thinned to a count that is no power of two lands top-p exactly on its
    threshold, which sampler_ref rightly calls undecided): no row is ever left without a finite score, and the reference alone
    stays under sampler_ref.UNDECIDED_CAP (tests/test_constraint_cpu.py).  Any allowed token leads to the next state."""
    from tcavt_amd.constraint import TokenConstraint

    ids = np.arange(V)
    cls = (ids % 3) + 3 * (ids % 5 == 0)  # 0 .. 5
    cls[[5, V // 2, V - 3, V - 1]] = 6
    cls[V // 3:V // 3 + 300] = 6  # the plateau row: its 300 equal top values stay together, so the cap still cuts an exact tie
    trans = np.full((3, 7), -1, dtype=np.int32)
    trans[0, [0, 3, 6]] = 1
    trans[1, [1, 4, 6]] = 2
    trans[2, [3, 4, 5, 6]] = 0
    return TokenConstraint(torch.from_numpy(cls.astype(np.int32)), torch.from_numpy(trans))


# (T, top_k, top_p, repetition_penalty, do_sample, seed): two greedy sets and a small part of sampler_ref.GRID, no_repeat = 0
SETS = ((1.0, 1, 1.0, 1.0, 0, 0), (1.0, 1, 1.0, 1.3, 0, 0), (0.7, 5, 0.9, 1.3, 1, 1234), (1.0, 40, 0.55, 1.0, 1, (1 << 40) + 77),
        (1.3, 256, 1.0, 1.3, 1, 1234), (1.0, 1, 0.9, 1.0, 1, 7))
STEPS = 6


V, CAP = 4100, 40  # V / 4 = 1025: a ragged last slice in both the mask and the two-stage sampler; a tail bitmap word


def sampler_inputs():
    """The eight base rows of sampler_ref.rows(V) and its histories: the inputs of the sampler chain tests."""
    scores, _ = SR.rows(V, extra=False)
    hist, hl = SR.histories(V, scores.shape[0], CAP)
    return scores, hist, hl


class Chain:
    """The reference side of ``mask -> sample -> advance`` over several steps of the batch form on fixed logits rows: per row the
    automaton state and the history; ``step(t, got)`` compares the tokens a kernel chose at step t (None: follow the reference's
    own) through the tally and moves on along the tokens actually taken."""

    def __init__(self, C, scores, hist, hist_len, cap, params, starts, tally):
        self.C, self.scores, self.cap, self.params, self.tally = C, scores, cap, params, tally
        self.hist = [SR.clamp_history(hist[r], hist_len[r], cap) for r in range(scores.shape[0])]
        self.state = [int(s) for s in starts]

    def step(self, t, got=None):
        T, k, p, rep, do_sample, seed = self.params
        taken = []
        for r in range(self.scores.shape[0]):
            ref = SR.Reference(masked(self.C, self.state[r], self.scores[r]), self.hist[r], rep, 0)
            c = ref.choose(bool(do_sample), T, k, p, seed, t, r)
            tok = c.token if got is None else int(got[r])
            self.tally.token(c, tok, (self.params, t, r))
            nxt = self.C.next(self.state[r], tok)
            assert nxt >= 0, f"row {r}, step {t}: token {tok} is not allowed in state {self.state[r]}"
            self.state[r] = nxt
            if len(self.hist[r]) < self.cap:
                self.hist[r].append(tok)
            taken.append(tok)
        return taken
