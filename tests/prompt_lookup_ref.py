"""Host references of prompt-lookup speculative decoding, shared by the tests of its kernels and of its host code.

``draft``        the draft rule in plain Python: for n from min(m, len - 1) down to 1, the earliest window that equals the last n
                 ids and has something behind it; up to k ids from right behind it, cut at the end.  No match: [].
``draft_rows``   what tcavt_ngram_draft writes for S sequences: n_draft [S], cur_rows [S * (k + 1)], pos_rows [S * (k + 1)].
``sequential``   the plain loop over a deterministic next_token(history, step): N tokens, ending on a token of ``ends``.
``speculative``  the same tokens by draft -> verify -> commit with any draft source: per step the leading drafts that equal the
                 tokens next_token would have chosen are accepted and one more token is committed behind them.
"""
import numpy as np


def draft(hist, k, m):
    hist = [int(t) for t in hist]
    L = len(hist)
    for n in range(min(m, L - 1), 0, -1):
        tail = hist[L - n:]
        for i in range(L - n):  # (i = L - n is the n-gram itself: nothing behind it)
            if hist[i:i + n] == tail:
                return hist[i + n:min(i + n + k, L)]
    return []


def draft_rows(history, hist_len, cur, pos, finished, k, m, pad):
    """history int64 [S, cap], hist_len / pos / finished [S], cur [S] -> (n_draft int32 [S], cur_rows int64 [S * T], pos_rows
    int32 [S * T]) with T = k + 1"""
    S, T = len(cur), k + 1
    n_draft = np.zeros(S, np.int32)
    cur_rows = np.full(S * T, pad, np.int64)
    pos_rows = np.zeros(S * T, np.int32)
    for s in range(S):
        d = [] if finished[s] else draft(history[s][:min(max(int(hist_len[s]), 0), history.shape[1])], k, m)
        n_draft[s] = len(d)
        cur_rows[s * T] = cur[s]
        cur_rows[s * T + 1:s * T + 1 + len(d)] = d
        pos_rows[s * T:(s + 1) * T] = int(pos[s]) + np.arange(T)
    return n_draft, cur_rows, pos_rows


def sequential(next_token, prompt, N, ends=()):
    hist, out = list(prompt), []
    for step in range(N):
        t = next_token(hist, step)
        out.append(t)
        hist.append(t)
        if t in ends:
            break
    return out


def speculative(next_token, prompt, N, source, k, ends=()):
    """-> (tokens, [(drafted, accepted, committed) per step]).  ``source(history, k)`` -> up to k draft ids.  The first token is
    the plain one (the prefill's); every later step verifies its draft position by position."""
    hist, out, log = list(prompt), [], []
    t = next_token(hist, 0)
    out.append(t)
    hist.append(t)
    done = t in ends or len(out) == N
    while not done:
        d = list(source(hist, k))[:k]
        accepted = committed = 0
        for j in range(len(d) + 1):
            t = next_token(hist, len(out))
            out.append(t)
            hist.append(t)
            committed += 1
            done = t in ends or len(out) == N
            if done or j == len(d) or t != d[j]:
                break
            accepted += 1
        log.append((len(d), accepted, committed))
    return out, log
