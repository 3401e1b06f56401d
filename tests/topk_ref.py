"""Float64 reference of the top-k alternatives (tcavt_logprob_topk) and the synthetic rows of its tests.

    lp  = x64 - max - log sum exp(x64 - max)        on the fp32 logits bits cast to float64
    ids = the k first ids by (value descending, id ascending)

The order is decided on the fp32 inputs themselves (the cast to float64 is exact and monotone), so the ids must be EQUAL to the
reference: no margin.  The values share the bar of tests/logprob_ref.py (|got - ref| <= 1e-5 + 2^-22 |ref|; derivation there):
the kernel's arithmetic is that of tcavt_logprob_finish on the same 16 partials."""
import numpy as np

from tests import logprob_ref as LR

bar, ratio = LR.bar, LR.ratio  # (imported, not restated)


def ref_topk(x, k):
    """x: fp32 [V] -> (ids int64 [k], lp float64 [k]).  -0.0 == +0.0 and equal values go by id; -inf entries come last by id."""
    x32 = np.asarray(x, dtype=np.float32)
    x64 = x32.astype(np.float64)
    kth = np.partition(x64, x64.size - k)[x64.size - k]  # the k-th largest value: every entry of the list is >= it
    cand = np.flatnonzero(x64 >= kth)
    order = np.lexsort((cand, -x64[cand]))  # last key first: value descending, then id ascending
    ids = cand[order[:k]].astype(np.int64)
    m = x64.max()
    with np.errstate(divide="ignore"):
        lse = m + np.log(np.exp(x64 - m).sum())
    return ids, x64[ids] - lse


def is_sorted(ids, lps):
    """A list is in (log-probability descending, id ascending) order (-1 / -inf padding allowed at the end)."""
    for i in range(len(ids) - 1):
        a, b = float(lps[i]), float(lps[i + 1])
        if a < b or (a == b and ids[i] >= ids[i + 1] and ids[i + 1] >= 0):
            return False
    return True


# ---- the input kinds of tests/test_logprob_topk_gpu.py -------------------------------------------------------------------------
KINDS = ("normal", "quantised", "equal", "mostly_ninf", "planted")


def make_row(kind, V, k, seed):
    """One NaN-free fp32 row of V scores."""
    g = np.random.default_rng(977 * seed + V + 31 * k + KINDS.index(kind))
    if kind == "normal":
        return (3.0 * g.standard_normal(V)).astype(np.float32)
    if kind == "quantised":  # steps of 0.5: ties are frequent and cross slice boundaries; some zeros are negative zeros
        x = (np.round(2.0 * 3.0 * g.standard_normal(V)) / 2.0).astype(np.float32)
        x[(x == 0) & (g.random(V) < 0.5)] = np.float32(-0.0)
        return x
    if kind == "equal":  # ids must be 0 .. k - 1
        return np.full(V, np.float32(g.standard_normal() * 3.0), dtype=np.float32)
    if kind == "mostly_ninf":  # all but max(k - 2, 1) entries -inf: the trailing entries of the list are -inf in id order
        x = np.full(V, -np.inf, dtype=np.float32)
        keep = g.choice(V, size=max(k - 2, 1), replace=False)
        x[keep] = (3.0 * g.standard_normal(keep.size)).astype(np.float32)
        return x
    if kind == "planted":  # the same maximum at the first and last element of every slice and at id V - 1
        x = (3.0 * g.standard_normal(V)).astype(np.float32)
        for lo, hi in LR.slice_bounds(V):
            if hi > lo:
                x[lo] = x[hi - 1] = np.float32(50.0)
        x[V - 1] = np.float32(50.0)
        return x
    raise ValueError(kind)
