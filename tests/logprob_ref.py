"""Float64 reference and error bar of the generated tokens' log-probabilities (tcavt_logprob_begin / _finish).

    ref = x64[tok] - logsumexp(x64)          on the fp32 logits bits cast to float64
    bar: |got - ref| <= 1e-5 + 2^-22 * |ref|

The bar: the relative error of S = sum exp(x - M) is bounded by the rounding of the exponent arguments, <= 2^-24 * ln V, plus the
exp / log ulps and at most ~40 roundings for "<= 16 serial adds per thread + tree + 16 partials" (40 * 2^-24 = 2.4e-6 in log S);
the subtraction x_tok - M adds 2^-24 * |x_tok - M|, which |ref| bounds up to log S.  ``restate_fp32`` is an fp32 numpy
restatement of exactly the kernels' summation shape; ``serial_fp32`` the same with one serial sum per slice."""
import numpy as np

ABS, REL = 1e-5, 2.0 ** -22
G, T, E4 = 16, 1024, 4  # slices per row, threads per slice, groups of 4 elements per thread and round
VOCABS = (48, 1000, 1003, 128256, 262144)
SIGMAS = (1.0, 4.0, 12.0)


def ref_logprob(x, tok):
    """x: fp32 [V] (any array-like); -> float64 log_softmax(x)[tok]."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    m = x64.max()
    return float(x64[int(tok)] - (m + np.log(np.exp(x64 - m).sum())))


def bar(ref):
    return ABS + REL * abs(ref)


def ratio(got, ref):
    """|got - ref| in units of the bar (<= 1 passes)."""
    return abs(float(got) - float(ref)) / bar(ref)


def slice_bounds(V):
    """[(lo, hi)] element ranges of the 16 slices: whole groups of 4 elements, ceil(ceil(V / 4) / 16) groups per slice."""
    n4 = (V + 3) // 4
    chunk4 = (n4 + G - 1) // G
    return [(min(4 * g * chunk4, V), min(4 * min((g + 1) * chunk4, n4), V)) for g in range(G)]


def _slice_partial(xs, serial):
    """(max, sum exp(x - max)) of one slice in fp32.  The kernel's shape: thread t holds groups t, t + 1024, ... (4 per round), adds
    its <= 16 exps serially, the 64 lanes of a wave meet by xor-butterflies, the 16 waves in index order."""
    f = np.float32
    if xs.size == 0:
        return f(-np.inf), f(0.0)
    M, S = f(-np.inf), f(0.0)
    per_round = 4 * E4 * T
    for base in range(0, xs.size, per_round):
        part = xs[base:base + per_round]
        m = part.max()
        if serial:
            s = f(0.0)
            for v in np.exp(part - m, dtype=f):  # one thread, one element after the other
                s = f(s + v)
        else:
            pad = np.full(per_round, -np.inf, dtype=f)
            pad[:part.size] = part
            a = pad.reshape(E4, T, 4).transpose(1, 0, 2).reshape(T, 4 * E4)  # thread t: groups t + e * 1024
            ex = np.exp(a - m, dtype=f)
            acc = np.zeros(T, dtype=f)
            for j in range(4 * E4):
                acc = (acc + ex[:, j]).astype(f)
            w = acc.reshape(T // 64, 64)
            lane = np.arange(64)
            for o in (32, 16, 8, 4, 2, 1):
                w = (w + w[:, lane ^ o]).astype(f)
            s = w[0, 0]
            for k in range(1, T // 64):
                s = f(s + w[k, 0])
        Mn = max(M, m)
        S = f(f(S * np.exp(f(M - Mn), dtype=f)) + f(s * np.exp(f(m - Mn), dtype=f)))
        M = Mn
    return M, S


def _combine(x, tok, serial):
    f = np.float32
    x = np.asarray(x, dtype=f)
    parts = [_slice_partial(x[lo:hi], serial) for lo, hi in slice_bounds(x.size)]
    M = max(p[0] for p in parts)
    S = f(0.0)
    with np.errstate(invalid="ignore"):
        for m, s in parts:
            S = f(S + f(s * np.exp(f(m - M), dtype=f)))
    return float(f(f(x[int(tok)] - M) - np.log(S, dtype=f)))


def restate_fp32(x, tok):
    """The kernels' arithmetic in fp32 numpy (same slices, same order of additions)."""
    return _combine(x, tok, serial=False)


def serial_fp32(x, tok):
    """The same with a fully serial fp32 sum over each slice: what the bar is meant to exclude at large V."""
    return _combine(x, tok, serial=True)


def random_row(V, sigma, seed=0):
    return (np.random.default_rng(1000 * seed + V).standard_normal(V) * sigma).astype(np.float32)


# ---- the planted cases of tests/test_logprob_kernels_gpu.py: each is (scores fp32 [V], history list, processors, token expected,
# wrong reading) -- `wrong` is what a faulty design would compute, >= 1 away from the reference
def planted_positions(V):
    """Index of the one element at 0 among -40: the row's ends, and the neighbours of every slice boundary -- of ceil(V / 16) * g
    and of the kernels' own boundaries (whole groups of 4)."""
    c = -(-V // 16)
    pos = {0, 1, 2, 3, V - 4, V - 3, V - 2, V - 1}
    for g in range(1, 16):
        pos |= {c * g - 1, c * g, c * g + 1}
    for lo, hi in slice_bounds(V):
        pos |= {lo - 1, lo, lo + 1, hi - 1}
    return sorted(p for p in pos if 0 <= p < V)


def planted_single(V, p):
    x = np.full(V, -40.0, dtype=np.float32)
    x[p] = 0.0
    return x


def planted_cases(V):
    """Cases 2 to 4: -> [dict(name, scores fp32 [V], hist, penalty, ngram, min_new, eos, token, wrong)].  ``token`` is what the
    greedy selection must choose after the processors; ``wrong`` is the value of the faulty reading named in ``name``."""
    g = np.random.default_rng(5 + V)
    cases = []
    # 2a / 2b: the chosen token is in the history, penalised by 1.3, and still wins; its RAW score counts
    for tag, raw, field in (("positive", 10.0, 3.0), ("negative", -5.0, -12.0)):
        x = (field + 0.5 * g.standard_normal(V)).astype(np.float32)
        t = V // 3
        x[t] = raw
        pen = float(np.float32(1.3))
        seen = raw / pen if raw > 0 else raw * pen
        cases.append(dict(name=f"penalised token, {tag} raw score: penalised value read", scores=x, hist=[1, t, 2], penalty=1.3, ngram=0,
                          min_new=0, eos=-1, token=t, wrong=ref_logprob(x, t) - (raw - seen)))
    # 3: the n-gram ban removes the token with the largest mass; the normaliser includes it
    x = (-6.0 + 0.5 * g.standard_normal(V)).astype(np.float32)
    a, b, c = 5, V - 2, V // 2
    x[b], x[c] = 12.0, 10.0
    y = x.copy()
    y[b] = -np.inf
    cases.append(dict(name="n-gram ban: normaliser of the banned row", scores=x, hist=[a, b, 7, a], penalty=1.0, ngram=2, min_new=0,
                      eos=-1, token=c, wrong=ref_logprob(y, c)))
    # 4: the same for the min_new_tokens ban of EOS
    x = (-6.0 + 0.5 * g.standard_normal(V)).astype(np.float32)
    eos, c = V - 1, 11
    x[eos], x[c] = 12.0, 10.0
    y = x.copy()
    y[eos] = -np.inf
    cases.append(dict(name="min_new_tokens ban of EOS: normaliser of the banned row", scores=x, hist=[1, 2, 3], penalty=1.0, ngram=0,
                      min_new=2, eos=eos, token=c, wrong=ref_logprob(y, c)))
    return cases
