"""Float64 reference of the token sampler (csrc/sampler.hip: sample_kernel, sample_slice_kernel) and the comparer that
decides when an fp32 kernel may differ from it -- TEST INFRASTRUCTURE ONLY, numpy only.

Written from the definitions of the transformers processors (RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor,
TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper, in that order) and from the project's stated conventions, not from
the kernel.  Nothing of oracle/ is used but oracle/philox.py, the shared generator with its own golden test.

Processors, on one row:
  * hist_len is clamped to hist_cap; ids outside [0, V) are never penalised or banned (inside an n-gram they still compare as the
    integers they are);
  * repetition penalty, once per DISTINCT history id: x * p if x < 0 else x / p;
  * no-repeat n-gram: the token that followed an earlier occurrence of the last n - 1 ids is banned by -inf; n = 1 bans every id
    of the history; a history with len + 1 < n bans nothing;
  * every float parameter is the fp32 value the C struct carries (float(np.float32(1.2)), not 1.2).

Selection, in float64: v = x / T over the finite scores, ordered (value descending, index ascending); kept: the first k plus every
tie with the k-th value, capped at CAP = 256 in that order (the cap is the kernel's documented departure from transformers);
top-p drops the low tail whose probability, counted from the bottom and including the item, is <= 1 - top_p, at least one item
stays; u = (r >> 8) / 2^24 with r = word 0 of Philox4x32-10(counter = (step, row, 0x5A3B, 0), key = seed); the token is the inverse
CDF of u * sum over the kept items in that order.  Greedy: the first maximum.  A row with NO finite score gives token 0 in both
modes: that is what the kernel does today, pinned here.

Three margins say whether fp32 may legitimately choose otherwise:
  k_gap    relative gap between the k-th kept value and the first dropped one (0: an exact tie cut by the cap; inf: nothing dropped)
  p_margin smallest |tail - (1 - top_p)| over the top-p steps taken
  u_margin smallest distance of u * sum to an interior CDF boundary, relative to the sum
A case is DECIDED when k_gap is 0 or >= K_GAP = 1e-6 and the other two are >= MARGIN = 2e-5 (derived, not measured: an fp32 sum
of at most 256 positive terms carries at most 255 * 2^-24 = 1.5e-5 relative error, plus a few ulp of __expf per term).  A decided
case must give exactly the reference token.  An undecided case must give one of the tokens the reference yields when every
ambiguous comparison is resolved either way (target moved by +-MARGIN, top-p threshold moved by +-MARGIN, the borderline values in,
out, or in the opposite order).  At most UNDECIDED_CAP = 2 % of the cases of one test may be undecided: a condition, not a tolerance.

Two refinements of that rule, both reasoned: (1) an EXACT case -- every kept value equal, a power-of-two count of them, top_p >= 0.5
-- is decided whatever its margins, because fp32 computes every weight, sum and quotient of it without rounding (this is what lets
a tail that lands exactly on 1 - top_p tell `<=` from `<`); (2) a case whose chosen item has a kept neighbour within K_GAP of it
but not equal is undecided, with that neighbour among the alternatives: fp32 may see the two as a tie and order them by index.

Processed logits (the kernel edits them in place): the -inf pattern is equal, finite values are within 2^-23 relative of the
float64 value (one fp32 rounding plus one ulp), every element no processor touches is bit-equal to the input.
"""
import numpy as np

from oracle import philox

CAP = 256
K_GAP = 1e-6
MARGIN = 2e-5
UNDECIDED_CAP = 0.02
REL_PROCESSED = 2.0 ** -23
_HEAD = 384  # sorted prefix kept per row: > CAP + 1, so the first dropped value is always inside it


def f32(x):
    return float(np.float32(x))


def clamp_history(history, hist_len, hist_cap):
    n = max(0, min(int(hist_len), int(hist_cap)))
    return [int(t) for t in np.asarray(history).reshape(-1)[:n]]


def process_logits(scores, hist, repetition_penalty, no_repeat_ngram_size):
    """-> (x float64 [V], touched bool [V]) of one row; hist: the clamped history as a list of ints."""
    x = np.asarray(scores, dtype=np.float32).astype(np.float64)
    V = x.size
    touched = np.zeros(V, dtype=bool)
    h = np.asarray(hist, dtype=np.int64).reshape(-1)
    p = f32(repetition_penalty)
    if p != 1.0:
        ids = np.unique(h[(h >= 0) & (h < V)])
        with np.errstate(invalid="ignore"):
            x[ids] = np.where(x[ids] < 0, x[ids] * p, x[ids] / p)
        touched[ids] = True
    n = int(no_repeat_ngram_size)
    m = h.size - n + 1  # an n-gram of the history starts at 0 .. m - 1
    if n > 0 and m > 0:
        ok = np.ones(m, dtype=bool)
        for k in range(n - 1):
            ok &= h[k:k + m] == h[h.size - (n - 1) + k]
        t = h[n - 1:n - 1 + m][ok]
        t = t[(t >= 0) & (t < V)]
        x[t] = -np.inf
        touched[t] = True
    return x, touched


def uniform(seed, step, row):
    M = 0xFFFFFFFF
    c = philox.philox4x32_10(np.array([int(step) & M], np.uint32), np.array([int(row) & M], np.uint32), np.array([0x5A3B], np.uint32),
                             np.array([0], np.uint32), int(seed) & M, (int(seed) >> 32) & M)
    return (int(c[0][0]) >> 8) / 16777216.0


class Choice:
    __slots__ = ("token", "decided", "alts", "k_gap", "p_margin", "u_margin", "kept")

    def __init__(self, token, decided, alts, k_gap=np.inf, p_margin=np.inf, u_margin=np.inf, kept=None):
        self.token, self.decided, self.alts = int(token), bool(decided), alts
        self.k_gap, self.p_margin, self.u_margin, self.kept = k_gap, p_margin, u_margin, kept


def _rel_gap(a, b):
    s = max(abs(a), abs(b))
    return 0.0 if s == 0.0 else abs(a - b) / s


def _keep(v, ids, k, mode="normal"):
    """v, ids: the sorted prefix.  -> (kept positions' values, ids, k_gap).  mode 'in': every value within K_GAP of the k-th is
    kept; 'flip': the values within K_GAP of the k-th take the opposite order first."""
    n = v.size
    k = min(int(k), n)
    if mode != "normal":
        kth = v[k - 1]
        band = np.abs(v - kth) <= K_GAP * np.maximum(np.abs(v), abs(kth))
        lo, hi = int(np.argmax(band)), n - int(np.argmax(band[::-1]))
        if mode == "in":
            m = min(max(hi, k), CAP)
            return v[:m], ids[:m], 0.0
        seg = np.lexsort((ids[lo:hi], v[lo:hi]))  # value ascending, index ascending
        v = np.concatenate([v[:lo], v[lo:hi][seg], v[hi:]])
        ids = np.concatenate([ids[:lo], ids[lo:hi][seg], ids[hi:]])
    kth = v[k - 1]
    m = k
    while m < n and v[m] == kth:
        m += 1
    if m > CAP:
        gap = 0.0  # an exact tie cut by the cap
    elif m < n:
        gap = _rel_gap(kth, v[m])
    else:
        gap = np.inf
    m = min(m, CAP)
    return v[:m], ids[:m], gap


def _draw(vals, ids, top_p, u, dp=0.0, du=0.0):
    """-> (token, p_margin, u_margin, items left by top-p, position of the token) from the kept (vals, ids); dp / du move the top-p threshold / the target.
    An EXACT case -- every kept value equal, a power-of-two count, top_p >= 0.5 -- has weights 1, sums that are small integers and
    quotients j / n: fp32 computes each of them without rounding, so it cannot differ and both margins are infinite."""
    n = vals.size
    exact = bool((vals == vals[0]).all()) and n & (n - 1) == 0 and top_p >= 0.5
    w = np.exp(vals - vals[0])
    tot = w.sum()
    keep, p_margin = n, np.inf
    if top_p < 1.0 and n > 1:
        tails = np.cumsum((w / tot)[:0:-1])  # tail after items n - 1, n - 2, ... 1
        ok = tails <= (1.0 - top_p) + dp
        r = n - 1 if ok.all() else int(np.argmin(ok))  # steps that dropped an item
        keep = n - r
        p_margin = float(np.min(np.abs(tails[:r + 1] - (1.0 - top_p))))  # the step that stopped counts too
    cdf = np.cumsum(w[:keep])
    kt = cdf[-1]
    target = (u + du) * kt
    pick = min(int(np.searchsorted(cdf, target, side="right")), keep - 1)
    u_margin = float(np.min(np.abs(cdf[:-1] - target)) / kt) if keep > 1 else np.inf
    if exact:
        p_margin = u_margin = np.inf
    return int(ids[pick]), p_margin, u_margin, keep, pick


class Reference:
    """One row: scores + clamped history + processors -> processed scores (x, touched); choose() selects a token."""

    def __init__(self, scores, hist, repetition_penalty, no_repeat_ngram_size):
        self.scores = np.asarray(scores, dtype=np.float32)
        self.x, self.touched = process_logits(self.scores, hist, repetition_penalty, no_repeat_ngram_size)
        self._head = None

    def head(self):
        """(values, ids) of the first _HEAD finite scores (plus every tie with the last of them) in (value desc, index asc) order."""
        if self._head is None:
            x = self.x
            fin = np.flatnonzero(np.isfinite(x))
            if fin.size > _HEAD:
                cut = np.partition(x[fin], fin.size - _HEAD)[fin.size - _HEAD]
                fin = fin[x[fin] >= cut]
            order = np.lexsort((fin, -x[fin]))
            self._head = (x[fin][order], fin[order])
        return self._head

    def choose(self, do_sample, temperature=1.0, top_k=1, top_p=1.0, seed=0, step=0, row=0):
        xs, ids = self.head()
        if xs.size == 0:
            return Choice(0, True, {0})  # no finite score: token 0 in both modes (pinned; the kernel's behaviour today)
        if not do_sample:
            exact = xs == xs[0]
            band = np.abs(xs - xs[0]) <= K_GAP * abs(xs[0])  # fp32 may order these otherwise
            gap = np.inf if exact.all() else _rel_gap(xs[0], xs[int(np.argmin(exact))])
            return Choice(ids[0], bool((band == exact).all()), {int(i) for i in ids[band]}, k_gap=gap)
        T, P = f32(temperature), f32(top_p)
        v = xs / T
        if np.any((np.diff(v) == 0) & (np.diff(ids) < 0)):  # the division made a new tie: restore the index order
            o = np.lexsort((ids, -v))
            v, ids = v[o], ids[o]
        u = uniform(seed, step, row)
        kv, ki, k_gap = _keep(v, ids, top_k)
        token, p_margin, u_margin, keep, pick = _draw(kv, ki, P, u)
        decided = (k_gap == 0.0 or k_gap >= K_GAP) and p_margin >= MARGIN and u_margin >= MARGIN
        alts = {token}
        # a kept neighbour of the chosen item within K_GAP of it, but not equal: fp32 may see a tie and order the two by index
        for j in (pick - 1, pick + 1):
            if 0 <= j < keep and kv[j] != kv[pick] and _rel_gap(kv[j], kv[pick]) < K_GAP:
                decided = False
                alts.add(int(ki[j]))
        if not decided:
            for mode in ("normal", "in", "flip"):
                mv, mi, _ = _keep(v, ids, top_k, mode)
                for dp in (0.0, MARGIN, -MARGIN):
                    for du in (0.0, MARGIN, -MARGIN):
                        alts.add(_draw(mv, mi, P, u, dp, du)[0])
        return Choice(token, decided, alts, k_gap, p_margin, u_margin, kept=ki[:keep])

    def check_processed(self, got):
        """got: the row after the kernel's call (fp32).  Asserts the contract of the processed logits; -> worst error in fp32 ulps."""
        got = np.asarray(got, dtype=np.float32)
        ninf = np.isneginf(self.x)
        wrong = np.flatnonzero(np.isneginf(got) != ninf)
        assert wrong.size == 0, f"-inf pattern of the processed logits: ids {wrong[:8].tolist()} (banned in the reference: {ninf[wrong[:8]].tolist()})"
        assert not np.isnan(got).any() and not np.isposinf(got).any()
        same = ~self.touched
        assert np.array_equal(got[same].view(np.uint32), self.scores[same].view(np.uint32)), "an untouched logit changed"
        fin = ~ninf
        err = np.abs(got[fin].astype(np.float64) - self.x[fin])
        assert (err <= REL_PROCESSED * np.abs(self.x[fin])).all(), "processed logit beyond 2^-23 relative of float64"
        with np.errstate(invalid="ignore", divide="ignore"):
            ulps = err / np.spacing(np.abs(self.x[fin]).astype(np.float32)).astype(np.float64)
        return float(np.nanmax(ulps)) if ulps.size else 0.0


class Tally:
    """The comparer over the cases of one test."""

    def __init__(self, name):
        self.name, self.n, self.undecided, self.bad, self.ulps = name, 0, 0, [], 0.0

    def token(self, choice, got, label):
        self.n += 1
        if choice.decided:
            if int(got) != choice.token:
                self.bad.append((label, "decided", int(got), choice.token, choice.k_gap, choice.p_margin, choice.u_margin))
        else:
            self.undecided += 1
            if int(got) not in choice.alts:
                self.bad.append((label, "undecided", int(got), sorted(choice.alts), choice.k_gap, choice.p_margin, choice.u_margin))

    def processed(self, ref, got):
        self.ulps = max(self.ulps, ref.check_processed(got))

    @property
    def share(self):
        return self.undecided / max(self.n, 1)

    def ok(self):
        return not self.bad and self.undecided <= UNDECIDED_CAP * self.n

    def report(self):
        return (f"{self.name}: {self.n} cases, {self.undecided} undecided ({100.0 * self.share:.2f} %), "
                f"worst processed-logit error {self.ulps:.3f} ulp, {len(self.bad)} mismatches")

    def finish(self):
        print("\n[sampler_bounds] " + self.report())
        assert not self.bad, (self.name, len(self.bad), self.bad[:5])
        assert self.undecided <= UNDECIDED_CAP * self.n, (self.name, self.undecided, self.n)


# ---------------------------------------------------------------------------------------------------------------------
# inputs shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
TEMPERATURES, TOP_KS, TOP_PS = (0.7, 1.0, 1.3), (1, 5, 40, 256), (0.55, 0.9, 1.0)
SEED_STEPS = ((1234, 3), ((1 << 40) + 77, 11))  # (seed, step); the second seed is above 2^32: seed_hi counts
GRID = [(T, k, p) for T in TEMPERATURES for k in TOP_KS for p in TOP_PS]
PROCESSORS = ((1.3, 3), (1.0, 0), (1.3, 2), (1.0, 1))  # (repetition_penalty, no_repeat_ngram_size) the grid cycles through


def rows(V, extra=True):
    """The eight seeded rows of a vocabulary -- the six awkward rows of test_two_stage_token_selection_equals_the_one_stage_form,
    one flat, one peaked -- and, where V allows, three more: the top value 100 times in each of the 16 slices, one finite outlier
    at -1e30 under ordinary scores, no finite score at all.  -> (scores fp32 [R, V], names)."""
    g = np.random.default_rng(1000003 + V)
    x = (g.standard_normal((8, V)) * 3.0).astype(np.float32)
    x[1] = np.round(x[1] * 2) / 2
    x[2] = 1.25
    x[3] = -np.inf
    x[3, [5, V // 2, V - 1]] = (0.5, 2.0, 2.0)
    x[4] = -np.inf
    x[4, V - 3] = -7.0
    x[5, V // 3:V // 3 + 300] = x[5].max() + 1.0
    x[6] = (g.standard_normal(V) * 0.05).astype(np.float32)
    x[7] = (g.standard_normal(V) * 12.0).astype(np.float32)
    names = ["random", "half-steps", "constant", "three finite", "one finite", "plateau", "flat", "peaked"]
    if extra:
        more = (g.standard_normal((3, V)) * 3.0).astype(np.float32)
        more[1, V // 5] = -1e30
        more[2] = -np.inf
        names += ["outlier -1e30", "nothing finite"]
        if V % 4 == 0 and V >= 4096:  # 100 copies of the top value in each slice of ceil(V / 4 / 16) * 4 scores
            chunk = (V // 4 + 15) // 16 * 4
            top = more[0].max() + 2.0
            for s in range(16):
                lo, hi = s * chunk, min((s + 1) * chunk, V)
                assert hi - lo >= 100
                more[0, lo + (np.arange(100) * ((hi - lo) // 100))] = top
            names.append("100 ties per slice")
            more = more[[1, 2, 0]]
        else:
            more = more[1:]
        x = np.concatenate([x, more])
    return x, names


def histories(V, R, cap=40):
    """Histories of 30 ids as the equality test builds them: random ids, and in row 0 repeats and n-gram matches near V - 1;
    then ids at 0 and V - 1, ids out of range, a banned token that is also penalised, a ban in another slice than the penalty."""
    g = np.random.default_rng(77 + V)
    h = g.integers(0, V, size=(R, cap)).astype(np.int64)
    h[:, 30:] = 0
    h[0, :30] = np.arange(30) % 7 + (V - 8)
    if R > 1:  # ends on (a, b): earlier (a, b, c) bans c under n = 3, (b, d) bans d under n = 2; a, b, c, d are penalised too
        a, b, c, d = 0, V - 1, V // 2 + 1, 3
        h[1, :30] = [a, b, c, 7, b, d, -1, V, (1 << 31) + 5, a, b, c, 9, 9, 9, V - 1, 0, 11, 12, 13, b, d, 14, 15, -1, V, 16, 17, a, b]
    return h, np.full(R, 30, dtype=np.int32)
