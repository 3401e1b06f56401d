"""The cases of the per-request sampler tests (tests/test_sampler_per_request_gpu.py holds the kernels to them,
tests/test_per_request_reference_cpu.py runs the float64 reference alone over the same cases) -- TEST INFRASTRUCTURE ONLY, numpy
only.  Inputs are sampler_ref's: the eight seeded rows of a vocabulary, its histories, GRID, PROCESSORS and SEED_STEPS.

A CASE SET is one sampler call: eight logits rows, and per REQUEST its own (T, top_k, top_p, repetition_penalty,
no_repeat_ngram_size, do_sample, seed, eos).  Call j gives request i the grid point GRID[(j + 5 i) % 36], the processors
PROCESSORS[(i + j) % 4] and the seed of SEED_STEPS[(i + j) % 2] (one of them above 2^32); every fourth request is greedy.  top_k
runs through {1, 5, 40, 256} with the grid.

The three forms place the requests differently:
  batch   request = row; one step word for all rows (SEED_STEPS[j % 2]'s step)
  slots   slot s serves request OUT_ROW[s] (a permutation that is not the identity, into N_REQ = 10 requests) at its own step STEPS[s]
  rows    logits row g belongs to slot SLOT_OF_ROW[g] (one row has none: -1), which serves request OUT_ROW[slot] at STEPS[slot]
"""
import numpy as np

from tests import sampler_ref as SR

VOCABS = (512, 4100, 128256)
FORMS = ("batch", "slots", "rows")
N_ROWS = 8
N_REQ = 10
OUT_ROW = np.array([9, 2, 7, 0, 5, 3, 8, 1], dtype=np.int64)
STEPS = np.array([0, 3, 1, 7, 2, 5, 9, 4], dtype=np.int32)
SLOT_OF_ROW = np.array([3, 0, -1, 5, 1, 7, 2, 6], dtype=np.int32)
FIN0 = np.array([0, 0, 0, 0, 0, 0, 1, 0], dtype=np.int32)  # one finished state entry among the live ones: it chooses no token
PAD = 7
EOS_NONE = -1


def calls(V):
    """The call numbers j of a vocabulary: the whole grid at the small ones, a few at the real one."""
    return range(len(SR.GRID)) if V < 100000 else (0, 9, 18, 27)


def request_params(j, n_req=N_REQ):
    """-> list of n_req dicts (T, k, p, rep, ngram, do_sample, seed, eos) of call j."""
    out = []
    for i in range(n_req):
        T, k, p = SR.GRID[(j + 5 * i) % len(SR.GRID)]
        rep, ngram = SR.PROCESSORS[(i + j) % len(SR.PROCESSORS)]
        seed = SR.SEED_STEPS[(i + j) % 2][0]
        out.append(dict(T=T, k=k, p=p, rep=rep, ngram=ngram, do_sample=int((i + j) % 4 != 3), seed=seed, eos=EOS_NONE))
    return out


_INPUTS = {}


def inputs(V):
    """(scores fp32 [8, V], history int64 [8, 40], hist_len int32 [8]) of a vocabulary, drawn once."""
    if V not in _INPUTS:
        scores, _ = SR.rows(V, extra=False)
        hist, hl = SR.histories(V, N_ROWS)
        assert scores.shape[0] == N_ROWS
        _INPUTS[V] = (scores, hist, hl)
    return _INPUTS[V]


def placement(form, j):
    """-> list of (logits row, state entry, request, step) of the rows that take part in call j of a form."""
    if form == "batch":
        step = SR.SEED_STEPS[j % 2][1]
        return [(b, b, b, step) for b in range(N_ROWS)]
    if form == "slots":
        return [(s, s, int(OUT_ROW[s]), int(STEPS[s])) for s in range(N_ROWS)]
    return [(g, int(s), int(OUT_ROW[s]), int(STEPS[s])) for g, s in enumerate(SLOT_OF_ROW) if s >= 0]


_REFS = {}


def reference(V, row, entry, rep, ngram):
    """The float64 reference of logits row `row` on the history of state entry `entry`: computed once, never changed."""
    key = (V, row, entry, rep, ngram)
    if key not in _REFS:
        scores, hist, hl = inputs(V)
        _REFS[key] = SR.Reference(scores[row], SR.clamp_history(hist[entry], hl[entry], hist.shape[1]), rep, ngram)
    return _REFS[key]


def choices(V, form, j):
    """-> list of (logits row, state entry, request, step, params, Reference, Choice) of call j; a token is chosen -- and compared
    -- where FIN0[state entry] == 0."""
    prm = request_params(j)
    out = []
    for row, entry, req, step in placement(form, j):
        q = prm[req]
        ref = reference(V, row, entry, q["rep"], q["ngram"])
        out.append((row, entry, req, step, q, ref, ref.choose(q["do_sample"], q["T"], q["k"], q["p"], q["seed"], step, req)))
    return out
