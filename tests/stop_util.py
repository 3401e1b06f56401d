"""What the ending-rule tests share (tests/test_stop_rules_cpu.py, tests/test_stop_rules_gpu.py): the test's own restatement of
the ban before ``min_new_tokens`` and the cut of an unruled row at its first end."""
import numpy as np


def ban_scores(x, step, min_new_tokens, eos_token_id, stop_ids):
    """Scores of one row with the ban applied: while step < min_new_tokens, EOS (when >= 0) and every stop id are -inf (HF
    MinNewTokensLengthLogitsProcessor with eos_token_id = [eos, *stop_ids]); from step == min_new_tokens on, untouched.  A copy."""
    x = np.array(x, dtype=np.float32, copy=True)
    if step < min_new_tokens:
        ids = [int(t) for t in stop_ids] + ([int(eos_token_id)] if eos_token_id is not None and eos_token_id >= 0 else [])
        x[ids] = -np.inf
    return x


def cut_row(rules, tokens, eos_token_id, pad, budget=None):
    """An unruled row under `rules`: -> (tokens up to and including the ending one, pad behind; n_generated; reason).  A row no
    rule ends ran out: reason 4 at its full length."""
    toks = [int(t) for t in tokens]
    n, reason = rules.first_end(toks, eos_token_id, budget=budget)
    if reason == 0:
        n, reason = len(toks), 4
    return toks[:n] + [int(pad)] * (len(toks) - n), n, reason
