"""tcavt_ngram_draft against the plain-Python draft rule (tests/prompt_lookup_ref.py, which test_prompt_lookup_cpu.py holds to
HF's PromptLookupCandidateGenerator): n_draft, cur_rows and pos_rows are equal exactly.

The kernel stages nothing in LDS (it compares the int64 ids where they lie), so there is no staging limit; what changes with the
length is the number of windows a thread walks (256 threads per sequence), so the lengths sit on both sides of 256 and of 512:
1, 2, 3, 40, 255, 256, 257, 300, 511, 513, 700.  S in {1, 3, 8}, k in {1, 3, 7}, m in {1, 2, 8}; vocabularies of 3 .. 6 ids so that
matches are common, mapped into ids that include negative values and values >= 2^31 (two ids that differ only above bit 31, and
two that differ only in sign: a narrowed compare would confuse them); finished rows; hist_len beyond the capacity (clamped) and
0.  The outputs live between sentinel bands, and the inputs keep their bits."""
import numpy as np
import pytest
import torch

import prompt_lookup_ref as R

pytestmark = pytest.mark.gpu

I32, I64 = torch.int32, torch.int64
LENGTHS = [1, 2, 3, 40, 255, 256, 257, 300, 511, 513, 700]
IDS = [5, 5 + 2 ** 32, -5, 2 ** 31, 2 ** 31 + 2 ** 33, 0]  # 5 and 5 + 2^32 share their low word; -5 / 5; 2^31 and 2^31 + 2^33
PAD, BAND = 777, 16


def _case(S, k, m, seed):
    g = np.random.default_rng(seed)
    cap = max(LENGTHS) + 4
    hist = np.full((S, cap), -1, np.int64)
    hist_len = np.zeros(S, np.int32)
    for s in range(S):
        L = LENGTHS[(seed + s) % len(LENGTHS)]
        V = 3 + (seed + s) % 4
        body = g.integers(0, V, L)
        if s % 3 == 1 and L > 8:  # a long repeat: the tail is a copy of an earlier stretch, so n = m matches with a full draft
            body[-4:] = body[2:6]
        hist[s, :L] = np.array(IDS)[body]
        hist_len[s] = L
    finished = (np.arange(S) % 4 == 2).astype(np.int32)
    if S == 8:
        hist_len[6] = cap + 50  # clamped to the capacity (the row then ends in -1s, which match each other)
        hist_len[7] = 0
    cur = g.integers(0, 100, S).astype(np.int64) + 2 ** 40
    pos = g.integers(0, 1000, S).astype(np.int32)
    return hist, hist_len, cur, pos, finished


@pytest.mark.parametrize("m", [1, 2, 8])
@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("S", [1, 3, 8])
def test_draft_equals_the_reference(gpu, S, k, m):
    from tcavt_amd import ops

    dev = gpu["device"]
    T = k + 1
    n_some = 0
    for seed in range(4):
        hist, hist_len, cur, pos, finished = _case(S, k, m, seed * 7 + S + k)
        want_n, want_cur, want_pos = R.draft_rows(hist, hist_len, cur, pos, finished, k, m, PAD)
        n_some += int((want_n > 0).sum())
        ins = [torch.from_numpy(x).to(dev) for x in (hist, hist_len, cur, pos, finished)]
        keep = [t.clone() for t in ins]
        nbuf = torch.full((S + 2 * BAND,), -99, dtype=I32, device=dev)
        cbuf = torch.full((S * T + 2 * BAND,), -99, dtype=I64, device=dev)
        pbuf = torch.full((S * T + 2 * BAND,), -99, dtype=I32, device=dev)
        n_draft, cur_rows, pos_rows = nbuf[BAND:BAND + S], cbuf[BAND:BAND + S * T], pbuf[BAND:BAND + S * T]
        ops.ngram_draft(ins[0], ins[1], ins[2], ins[3], ins[4], k, m, PAD, n_draft, cur_rows, pos_rows)
        torch.cuda.synchronize()
        for a, b in zip(ins, keep):
            assert torch.equal(a, b), "an input was modified"
        for buf, n in ((nbuf, S), (cbuf, S * T), (pbuf, S * T)):
            assert bool((buf[:BAND] == -99).all()) and bool((buf[BAND + n:] == -99).all()), "write outside the outputs"
        assert n_draft.cpu().tolist() == want_n.tolist(), (seed, hist_len.tolist())
        assert cur_rows.cpu().tolist() == want_cur.tolist(), seed
        assert pos_rows.cpu().tolist() == want_pos.tolist(), seed
        assert all(want_n[s] == 0 for s in range(S) if finished[s])
    assert n_some > 0  # the cases do draft


def test_wide_ids_are_not_folded(gpu):
    """the tail (5, -5) occurs earlier only as (5 + 2^32, -5) and (5, 5): neither is a match for n = 2, and n = 1 finds -5"""
    from tcavt_amd import ops

    dev = gpu["device"]
    hist = np.array([[5 + 2 ** 32, -5, 11, 5, 5, 12, 5, -5]], np.int64)
    want = R.draft(hist[0], 3, 2)
    assert want == [11, 5, 5]
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    n_draft, cur_rows, pos_rows = z(1, I32), z(4, I64), z(4, I32)
    ops.ngram_draft(torch.from_numpy(hist).to(dev), torch.tensor([8], dtype=I32, device=dev), torch.tensor([-5], dtype=I64, device=dev),
                    z(1, I32), z(1, I32), 3, 2, PAD, n_draft, cur_rows, pos_rows)
    assert n_draft.tolist() == [3] and cur_rows.tolist() == [-5, 11, 5, 5] and pos_rows.tolist() == [0, 1, 2, 3]
