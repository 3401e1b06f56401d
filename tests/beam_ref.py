"""Float64 restatement of the beam search that tcavt_beam_select / tcavt_beam_reorder run (include/tcavt.h states the steps; they
restate HF 5.x GenerationMixin._beam_search with explicit masks instead of -1e9 additions).  tests/golden/tiny_beam.npz pins it
to HF's own results (tests/test_beam_reference_cpu.py); the GPU tests compare the kernels with it step by step.

Per prompt, K = 2 n.  ``search`` drives the whole search from a ``logits_fn(generated prefix) -> row``; ``candidates`` and
``advance`` are its two halves, usable on a state that came from elsewhere (the device's own fp32 state)."""
import numpy as np


def log_softmax64(row):
    x = np.asarray(row).astype(np.float64)
    m = x.max()
    return x - (m + np.log(np.exp(x - m).sum()))


def processed(row, history, penalty, ngram):
    """log_softmax of the raw row, then HF's processors ON the log-probabilities: RepetitionPenaltyLogitsProcessor over the ids of
    ``history`` (once per id), NoRepeatNGramLogitsProcessor over the same history.  float64 [V]."""
    lp = log_softmax64(row)
    hist = [int(t) for t in history]
    if penalty != 1.0:
        for t in sorted(set(hist)):
            if 0 <= t < lp.size:
                lp[t] = lp[t] * penalty if lp[t] < 0 else lp[t] / penalty
    if ngram > 0 and len(hist) + 1 >= ngram:
        tail = hist[len(hist) - (ngram - 1):] if ngram > 1 else []
        for i in range(len(hist) - ngram + 1):
            if hist[i:i + ngram - 1] == tail and 0 <= hist[i + ngram - 1] < lp.size:
                lp[hist[i + ngram - 1]] = -np.inf
    return lp


class State:
    """n running beams (tokens, run_score, live) and the finished store (<= n entries (tokens, score), best first)."""

    def __init__(self, n):
        self.n = n
        self.tokens = [[] for _ in range(n)]
        self.run_score = [0.0] * n
        self.live = [j == 0 for j in range(n)]
        self.fin = []
        self.unsat, self.done = True, False


def candidates(lp_rows, run_score, live, n, k=None):
    """The k (default K = 2 n) first of all live (j, token) by (acc = lp + run_score[j] descending, j * V + token ascending)
    -> [(parent, token, acc)].  lp_rows[j]: the processed log-probabilities of beam j (ignored for a dead beam)."""
    k = 2 * n if k is None else k
    V = next(np.asarray(r).size for j, r in enumerate(lp_rows) if live[j])
    acc = np.full((n, V), -np.inf)
    valid = np.zeros((n, V), dtype=bool)
    for j in range(n):
        if live[j]:
            acc[j] = np.asarray(lp_rows[j], dtype=np.float64) + run_score[j]
            valid[j] = True
    flat = acc.reshape(-1)
    keys = np.nonzero(valid.reshape(-1))[0]
    if keys.size > 4 * k:  # everything at or above the k-th largest value, then the exact order of those
        kth = np.partition(flat[keys], keys.size - k)[keys.size - k]
        keys = keys[flat[keys] >= kth]
    order = keys[np.lexsort((keys, -flat[keys]))][:k]
    return [(int(q // V), int(q % V), float(flat[q])) for q in order]


def advance(state, cands, s, N, eos, len_pow_s, early, div=lambda acc, lp: acc / lp, pad=0):
    """Steps 3 to 7 on ``state`` (changed in place) from the sorted candidates of step s -> dict(stop, parent, token) of the step.
    ``div``: the division that makes a finished score (float64 here; the device's is one fp32 division)."""
    n = state.n
    stop = [tok == eos or s + 1 == N for _, tok, _ in cands]
    new = [(p, t, a) for (p, t, a), st in zip(cands, stop) if not st][:n]
    all_flag = len(state.fin) == n
    admit = state.unsat and not (all_flag and early)
    merged = list(state.fin)
    for k, ((p, t, a), st) in enumerate(zip(cands, stop)):
        if st and k < n and admit:
            merged.append((state.tokens[p] + [t], div(a, len_pow_s)))
    order = sorted(range(len(merged)), key=lambda i: (-merged[i][1], i))[:n]
    state.fin = [merged[i] for i in order]
    old_tokens = state.tokens
    state.tokens = [old_tokens[p] + [t] for p, t, _ in new] + [[] for _ in range(n - len(new))]
    state.run_score = [a for _, _, a in new] + [-np.inf] * (n - len(new))
    state.live = [True] * len(new) + [False] * (n - len(new))
    some_false = len(state.fin) < n
    best_beats = bool(new) and div(new[0][2], len_pow_s) > min(sc for _, sc in state.fin) if state.fin else False
    state.unsat = state.unsat and (some_false or best_beats)
    state.done = (not state.unsat) or (len(state.fin) == n and early) or all(stop)
    return dict(stop=stop, parent=[p for p, _, _ in new] + list(range(len(new), n)), token=[t for _, t, _ in new] + [pad] * (n - len(new)))


def len_pow_table(N, length_penalty, dtype=np.float64):
    return np.array([float(s + 1) ** float(length_penalty) for s in range(N)], dtype=np.float64).astype(dtype)


def search(logits_fn, prompt_ids, n, N, eos=None, penalty=1.0, ngram=0, length_penalty=1.0, early=False, pad=0):
    """-> dict(sequences int64 [n, N] (pad behind a hypothesis), scores float64 [n], lengths, steps, trace): the n finished hypotheses
    best first and, per step, the K candidates [(parent, token, acc)].  logits_fn(tuple of generated tokens) -> the raw row."""
    eos = -1 if eos is None else int(eos)
    lpow = len_pow_table(N, length_penalty)
    state, trace = State(n), []
    for s in range(N):
        rows = [processed(logits_fn(tuple(state.tokens[j])), list(prompt_ids) + state.tokens[j], penalty, ngram) if state.live[j] else None
                for j in range(n)]
        cands = candidates(rows, state.run_score, state.live, n)
        trace.append(cands)
        advance(state, cands, s, N, eos, float(lpow[s]), early, pad=pad)
        if state.done:
            break
    seqs = np.full((n, N), pad, dtype=np.int64)
    for i, (toks, _) in enumerate(state.fin):
        seqs[i, :len(toks)] = toks
    return dict(sequences=seqs, scores=np.array([sc for _, sc in state.fin], dtype=np.float64),
                lengths=np.array([len(t) for t, _ in state.fin]), steps=len(trace), trace=trace)
