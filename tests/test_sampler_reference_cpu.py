"""The float64 sampler reference (tests/sampler_ref.py) and its comparer, proven on the CPU before the kernels meet them:

  * the reference's processed scores and kept set equal what transformers' own processor classes give in float64 (rows whose tie
    set exceeds 256 are left out: the stated departure), and agree with the `processed` / `warped` arrays of tiny_generation.npz;
  * the fp32 oracle (oracle/generation.py) passes the comparer on the GPU tests' grid at the CPU-affordable sizes, within the cap;
  * eleven mutants of the oracle -- each a one-line change of the copy below -- FAIL it on those same inputs.
"""
import os

import numpy as np
import pytest

from oracle import generation as G
from oracle import philox
from tests import sampler_ref as SR
from tests.util import GOLDEN

VS = (512, 1002, 4100)
_REFS = {}


def _reference(V, r, rep, ngram):
    key = (V, r, rep, ngram)
    if key not in _REFS:
        x, _ = SR.rows(V)
        h, hl = SR.histories(V, x.shape[0])
        _REFS[key] = SR.Reference(x[r], SR.clamp_history(h[r], hl[r], h.shape[1]), rep, ngram)
    return _REFS[key]


def _cases():
    """(V, row, hist, rep, ngram, do_sample, T, k, p, seed, step) over the grid of the GPU tests, plus the exact-threshold cases
    (constant and plateau rows, top_k 256, a dyadic 1 - top_p: the tail lands ON the threshold; see sampler_ref's EXACT rule)."""
    for V in VS:
        x, _ = SR.rows(V)
        h, hl = SR.histories(V, x.shape[0])
        for r in range(x.shape[0]):
            hist = SR.clamp_history(h[r], hl[r], h.shape[1])
            for gi, (T, k, p) in enumerate(SR.GRID):
                rep, ngram = SR.PROCESSORS[gi % len(SR.PROCESSORS)]
                for seed, step in SR.SEED_STEPS:
                    yield V, r, x[r], hist, rep, ngram, 1, T, k, p, seed, step
            for rep, ngram in SR.PROCESSORS:
                yield V, r, x[r], hist, rep, ngram, 0, 1.0, 1, 1.0, 0, 0
            if r in (2, 5):
                for p in (0.5, 0.75):
                    for seed, step in SR.SEED_STEPS:
                        yield V, r, x[r], hist, 1.0, 0, 1, 1.0, 256, p, seed, step


# ---------------------------------------------------------------------------------------------------------------------
# a copy of oracle.generation's processors and selection with one switch per mutant (mut = None: the oracle itself)
# ---------------------------------------------------------------------------------------------------------------------
MUTANTS = ("top_p_lt", "top_p_tail_excludes_item", "penalty_per_occurrence", "penalty_always_divides", "ties_dropped",
           "ties_by_descending_index", "greedy_last_maximum", "ngram_tail_one_short", "philox_word_1", "uniform_low_23_bits",
           "row_step_swapped")


def _process(scores, history, rep, n, mut):
    x = np.array(scores, dtype=np.float32, copy=True)
    hist = [int(t) for t in history]
    if rep != 1.0:
        for t in (hist if mut == "penalty_per_occurrence" else sorted(set(hist))):
            if 0 <= t < x.size:
                x[t] = x[t] * np.float32(rep) if (x[t] < 0 and mut != "penalty_always_divides") else x[t] / np.float32(rep)
    if n > 0 and len(hist) + 1 >= n:
        short = 1 if mut == "ngram_tail_one_short" else 0
        tail = hist[len(hist) - (n - 1) - short:len(hist) - short] if n > 1 else []
        for i in range(len(hist) - n + 1):
            if hist[i:i + n - 1] == tail and 0 <= hist[i + n - 1] < x.size:
                x[hist[i + n - 1]] = -np.inf
    return x


def _select(x, do_sample, T, top_k, top_p, seed, step, row, mut):
    if not do_sample:
        return int(x.size - 1 - np.argmax(x[::-1])) if mut == "greedy_last_maximum" else int(np.argmax(x))
    if not np.isfinite(x).any():
        return 0
    v = x.astype(np.float32) * np.float32(1.0 / np.float32(T))
    idx = np.arange(v.size)
    order = np.lexsort((-idx if mut == "ties_by_descending_index" else idx, -v))
    order = order[np.isfinite(v[order])]
    k = min(top_k, order.size)
    kth = v[order[k - 1]]
    keep = order[:k] if mut == "ties_dropped" else order[v[order] >= kth][:256]
    w = np.exp((v[keep] - v[keep[0]]).astype(np.float32)).astype(np.float32)
    if top_p < 1.0:
        tot = np.float32(0)
        for e in w:
            tot = np.float32(tot + e)
        tail, cut = np.float32(0), keep.size
        thr = np.float32(1.0) - np.float32(top_p)
        for j in range(keep.size - 1, 0, -1):
            nxt = np.float32(tail + np.float32(w[j] / tot))
            t = tail if mut == "top_p_tail_excludes_item" else nxt
            if (t < thr) if mut == "top_p_lt" else (t <= thr):
                cut = j
            else:
                break
            tail = nxt
        keep, w = keep[:cut], w[:cut]
    c0, c1 = (row, step) if mut == "row_step_swapped" else (step, row)
    c = philox.philox4x32_10(np.array([c0], np.uint32), np.array([c1], np.uint32), np.array([0x5A3B], np.uint32),
                             np.array([0], np.uint32), seed & 0xFFFFFFFF, seed >> 32)
    r = int(c[1 if mut == "philox_word_1" else 0][0])
    uni = np.float32((r & 0x7FFFFF) * (1.0 / 8388608.0)) if mut == "uniform_low_23_bits" else np.float32((r >> 8) * (1.0 / 16777216.0))
    kt = np.float32(0)
    for e in w:
        kt = np.float32(kt + e)
    u = np.float32(uni * kt)
    acc = np.float32(0)
    for j in range(keep.size):
        acc = np.float32(acc + w[j])
        if u < acc:
            return int(keep[j])
    return int(keep[-1])


def _run(mut, use_oracle=False, stop_at_first=False):
    """The copy (or the oracle) through the comparer over every case -> Tally."""
    tally = SR.Tally(mut or ("oracle" if use_oracle else "copy"))
    done = set()
    for V, r, scores, hist, rep, ngram, do_sample, T, k, p, seed, step in _cases():
        ref = _reference(V, r, rep, ngram)
        x = G.process_logits(scores, hist, rep, ngram) if use_oracle else _process(scores, hist, rep, ngram, mut)
        if (V, r, rep, ngram) not in done:
            done.add((V, r, rep, ngram))
            try:
                tally.processed(ref, x)
            except AssertionError as e:
                tally.bad.append(((V, r, rep, ngram), "processed", str(e)))
        if use_oracle:
            got = G.select_token(x, bool(do_sample), T, k, p, seed=seed, step=step, row=r)
        else:
            got = _select(x, do_sample, T, k, p, seed, step, r, mut)
        tally.token(ref.choose(do_sample, T, k, p, seed, step, r), got, (V, r, rep, ngram, do_sample, T, k, p, seed, step))
        if stop_at_first and tally.bad:
            break
    return tally


def test_the_oracle_passes_the_comparer_within_the_cap():
    t = _run(None, use_oracle=True)
    t.finish()
    assert t.n > 1400 and t.ulps <= 1.0


def test_the_copy_without_a_mutation_is_the_oracle():
    for V, r, scores, hist, rep, ngram, do_sample, T, k, p, seed, step in _cases():
        if (r + k) % 3:  # a third of the cases: the copy differs from the oracle by its switches only
            continue
        a = G.process_logits(scores, hist, rep, ngram)
        b = _process(scores, hist, rep, ngram, None)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert G.select_token(a, bool(do_sample), T, k, p, seed=seed, step=step, row=r) == _select(b, do_sample, T, k, p, seed, step, r, None)


@pytest.mark.parametrize("mut", MUTANTS)
def test_every_mutant_fails_the_comparer(mut):
    t = _run(mut, stop_at_first=True)
    assert t.bad, f"the mutant {mut} survived {t.n} cases"
    assert t.bad[0][1] in ("decided", "processed"), t.bad[0]  # rejected by a decided case, not by an odd alternative


def test_a_uniform_from_the_top_23_bits_is_below_what_any_decided_case_can_see():
    """(r >> 9) / 2^23 differs from (r >> 8) / 2^24 by at most 2^-24 = 6e-8: three hundred times inside MARGIN, so every case in
    which it could change the token is undecided by definition.  The mutant above therefore takes its 23 bits from the LOW end."""
    for r in (0, 1, 0x1FF, 0x80000100, 0xFFFFFFFF, 0x12345678):
        assert abs((r >> 9) / 2.0 ** 23 - (r >> 8) / 2.0 ** 24) <= 2.0 ** -24 < SR.MARGIN / 300


# ---------------------------------------------------------------------------------------------------------------------
# the reference against transformers
# ---------------------------------------------------------------------------------------------------------------------
def _hf_processed_and_kept(scores, hist, rep, ngram, T, k, p):
    torch = pytest.importorskip("torch")
    lp = pytest.importorskip("transformers").generation.logits_process
    ids = torch.tensor([hist], dtype=torch.int64)
    s = torch.tensor(np.asarray(scores, dtype=np.float64)[None])
    if SR.f32(rep) != 1.0:
        s = lp.RepetitionPenaltyLogitsProcessor(SR.f32(rep))(ids, s)
    if ngram > 0:
        s = lp.NoRepeatNGramLogitsProcessor(ngram)(ids, s)
    processed = s[0].numpy().copy()
    s = lp.TemperatureLogitsWarper(SR.f32(T))(ids, s)
    s = lp.TopKLogitsWarper(k)(ids, s)
    s = lp.TopPLogitsWarper(SR.f32(p))(ids, s)
    return processed, np.flatnonzero(np.isfinite(s[0].numpy()))


def test_reference_equals_the_transformers_processors_in_float64():
    pytest.importorskip("transformers")
    V = 512
    x, names = SR.rows(V)
    h, hl = SR.histories(V, x.shape[0])
    n = 0
    for r, name in enumerate(names):
        if name == "nothing finite":  # transformers has no answer there (softmax of -inf everywhere)
            continue
        hist = [t for t in SR.clamp_history(h[r], hl[r], h.shape[1]) if 0 <= t < V]  # its gather / scatter need ids in range
        for rep, ngram in SR.PROCESSORS + ((1.2, 3),):
            ref = SR.Reference(x[r], hist, rep, ngram)
            for T, k, p in SR.GRID:
                processed, kept = _hf_processed_and_kept(x[r], hist, rep, ngram, T, k, p)
                assert np.array_equal(processed, ref.x, equal_nan=False), (name, rep, ngram)
                c = ref.choose(1, T, k, p, seed=1, step=0, row=r)
                vs = np.sort(ref.x[np.isfinite(ref.x)])[::-1]
                kk = min(k, vs.size)
                if np.count_nonzero(vs >= vs[kk - 1]) > SR.CAP:  # the tie set exceeds the cap: the stated departure
                    continue
                if c.p_margin < 1e-9:  # (its softmax and cumsum round differently in the last bits)
                    continue
                # the same VALUES always; the same ids unless top-p cut through a group of equal values (which member of a tie
                # goes first is this project's convention -- index ascending -- and an accident of torch.sort there)
                assert np.array_equal(np.sort(ref.x[c.kept]), np.sort(processed[kept])), (name, rep, ngram, T, k, p)
                if np.count_nonzero(ref.x == ref.x[c.kept].min()) == np.count_nonzero(ref.x[c.kept] == ref.x[c.kept].min()):
                    assert np.array_equal(np.sort(c.kept), kept), (name, rep, ngram, T, k, p)
                n += 1
    assert n > 1000


def test_reference_agrees_with_the_golden_processed_and_warped_arrays():
    fx = dict(np.load(os.path.join(GOLDEN, "tiny_generation.npz"), allow_pickle=False))
    for r in range(fx["scores"].shape[0]):
        hist = SR.clamp_history(fx["hist"][r], fx["hist_len"][r], fx["hist"].shape[1])
        ref = SR.Reference(fx["scores"][r], hist, 1.2, 3)
        ref.check_processed(fx["processed"][r])
        c = ref.choose(1, 0.9, 40, 0.9, seed=1, step=0, row=r)
        assert c.p_margin > 1e-6
        assert np.array_equal(np.sort(c.kept), np.flatnonzero(np.isfinite(fx["warped"][r]))), r
