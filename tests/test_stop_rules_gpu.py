"""Ending rules on the GPU (tcavt_sample_tokens; generate_batch / generate_pool with stop_token_ids, stop_sequences,
min_new_tokens, poll_every, return_info).  The sampler on bare logits: all three forms (batch, slots, rows), one-stage and
two-stage, V = 128256 and V = 1003 (which takes the one-stage form even with a workspace); the expected token is
oracle.generation.select_token on scores the test banned itself (tests/stop_util.ban_scores), the expected state follows from
StopRules.first_end.  The model: a run with rules equals the unruled run cut by first_end.  Every comparison is on token ids, flags
and counts, and is exact."""
import numpy as np
import pytest
import torch

from tests.stop_util import ban_scores, cut_row
from tests.util import load_generation_case

pytestmark = pytest.mark.gpu

PAD, SENT, OUT_SENT = 9, -7, -5
TOP, SECOND = 50.0, 40.0  # planted scores: far above the random rows (|x| < ~15), so the planted order decides the token
OUT_ROWS = [3, 0, 7, 2, 9, 1]
FORMS = [(128256, False), (128256, True), (1003, False), (1003, True)]
FORM_IDS = ["V128256-one_stage", "V128256-two_stage", "V1003-one_stage", "V1003-workspace_one_stage"]
_BASE = {}


def _base(V):
    """Six fp32 random rows, computed once per V and never changed."""
    if V not in _BASE:
        _BASE[V] = (torch.randn(6, V, generator=torch.Generator().manual_seed(V)) * 3.0).numpy()
    return _BASE[V]


def _spec(prompt, gen, plant=None, fin=0, budget=1 << 20):
    return dict(prompt=list(prompt), gen=list(gen), plant=dict(plant or {}), fin=fin, budget=budget)


def _run(dev, mode, V, two_stage, specs, rules, *, eos=-1, do_sample=0, seed=1, lrows=None, expect_rules=None, seq_len=None):
    """One sampler call on planted state, checked against the oracle.  specs: one per STATE row (equal gen lengths); lrows: the
    state row of every logits row (rows form: the map, which may hold pad entries).  -> the arrays after the call."""
    from oracle import generation as G
    from tcavt_amd import capi, ops

    i32, i64 = torch.int32, torch.int64
    n_state = len(specs)
    lrows = list(range(n_state)) if lrows is None else list(lrows)
    assert mode == "rows" or lrows == list(range(n_state))
    n_log = len(lrows)
    step0 = len(specs[0]["gen"])
    assert all(len(s["gen"]) == step0 for s in specs)
    cap = max(len(s["prompt"]) + len(s["gen"]) for s in specs) + 4
    slots = mode != "batch"
    out_rows = OUT_ROWS[:n_state] if slots else list(range(n_state))
    n_out = max(out_rows) + 1
    # ---- state
    hist = torch.zeros(n_state, cap, dtype=i64)
    for s, sp_ in enumerate(specs):
        t = sp_["prompt"] + sp_["gen"]
        hist[s, :len(t)] = torch.tensor(t, dtype=i64)
    hl = torch.tensor([len(s["prompt"]) + len(s["gen"]) for s in specs], dtype=i32)
    pos0 = torch.arange(n_state, dtype=i32) * 3 + 20
    st = dict(history=hist.to(dev), hist_len=hl.to(dev), step=torch.full((n_state if slots else 1,), step0, dtype=i32, device=dev),
              cur=torch.full((n_state,), -3, dtype=i64, device=dev), pos=pos0.to(dev),
              finished=torch.tensor([s["fin"] for s in specs], dtype=i32, device=dev),
              out=torch.full((n_out, 16), OUT_SENT, dtype=i64, device=dev))
    max_new = torch.tensor([s["budget"] for s in specs], dtype=i32, device=dev) if slots else None
    out_row = torch.tensor(out_rows, dtype=i64, device=dev) if slots else None
    slot_of_row = torch.tensor(lrows, dtype=i32, device=dev) if mode == "rows" else None
    # ---- logits
    base = _base(V)
    logits_h = np.stack([base[g].copy() for g in range(n_log)])
    for g, s in enumerate(lrows):
        if 0 <= s < n_state:
            for tok, val in specs[s]["plant"].items():
                logits_h[g, tok] = val
    logits = torch.from_numpy(logits_h).to(dev).clone()
    wsp = ops.sample_workspace(n_log, dev) if two_stage else None
    params = capi.SampleParams(0.9, 0.9, 1.0, 40, 0, int(do_sample), int(eos), PAD, seed)  # processors off: the rules are what differs
    d = rules.to(dev).records(n_out, dev)
    d.finish_reason.fill_(SENT)
    d.n_generated.fill_(SENT)
    if seq_len is not None:
        d.seq_len = torch.tensor(seq_len, dtype=i32, device=dev)
    before = {k: v.clone() for k, v in st.items()}
    ops.sample_tokens(logits, st["history"], st["hist_len"], params, st["step"], st["cur"], st["pos"], st["finished"], st["out"],
                      advance_pos=True, workspace=wsp, max_new=max_new, out_row=out_row, slot_of_row=slot_of_row, stop=d)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in st.items()}
    got.update(logits=logits.cpu().numpy(), reason=d.finish_reason.cpu(), n_gen=d.n_generated.cpu(), tokens={})
    # ---- expectations
    exp_rules = expect_rules if expect_rules is not None else rules
    want_out = torch.full((n_out, 16), OUT_SENT, dtype=i64)
    want_reason = torch.full((n_out,), SENT, dtype=i32)
    want_ngen = torch.full((n_out,), SENT, dtype=i32)
    touched = set()
    for g, s in enumerate(lrows):
        if not 0 <= s < n_state:  # a pad row of the rows form: nothing of it is written, its logits row included
            assert np.array_equal(got["logits"][g], logits_h[g]), (g, "pad row's logits")
            continue
        touched.add(s)
        sp_ = specs[s]
        row = out_rows[s]
        h0 = int(hl[s])
        if sp_["fin"]:
            assert int(got["cur"][s]) == PAD
            if slots:  # inert: nothing else is written
                for k in ("history", "hist_len", "step", "pos", "finished"):
                    assert torch.equal(got[k][s], before[k][s].cpu()), (s, k)
            else:      # the batch form pads a finished row (as without rules)
                want_out[row, step0] = PAD
                assert int(got["history"][s, h0]) == PAD and int(got["hist_len"][s]) == h0 + 1
            continue
        x = ban_scores(logits_h[g], step0, rules.min_new_tokens, eos, rules.stop_token_ids)
        tok = G.select_token(x, bool(do_sample), 0.9, 40, 0.9, seed=seed, step=step0, row=row)
        got["tokens"][s] = tok
        gen = sp_["gen"] + [tok]
        n, reason = exp_rules.first_end(gen, eos if eos >= 0 else None, budget=sp_["budget"] if slots else None)
        assert reason == 0 or n == len(gen), "test setup: the planted history already ends the request"
        want_out[row, step0] = tok
        assert int(got["cur"][s]) == tok == int(got["history"][s, h0]), (s, int(got["cur"][s]), tok)
        assert int(got["hist_len"][s]) == h0 + 1 and int(got["pos"][s]) == int(pos0[s]) + 1
        if slots:
            assert int(got["step"][s]) == step0 + 1
        assert int(got["finished"][s]) == (1 if reason else 0), (s, reason, tok)
        if reason:
            want_reason[row], want_ngen[row] = reason, step0 + 1
        # the ban is in the row, in place, and nothing else of the row changed (the processors are off)
        assert np.array_equal(np.isinf(got["logits"][g]), np.isinf(x)), (g, "banned ids")
        assert np.array_equal(got["logits"][g][np.isfinite(x)], x[np.isfinite(x)])
    for s in range(n_state):
        if s not in touched:  # a slot no logits row maps to
            for k in ("history", "hist_len", "step", "pos", "finished", "cur"):
                assert torch.equal(got[k][s], before[k][s].cpu()), (s, k)
    if not slots:
        assert int(got["step"][0]) == step0 + 1
    assert torch.equal(got["out"], want_out)
    assert torch.equal(got["reason"], want_reason), (got["reason"].tolist(), want_reason.tolist())
    assert torch.equal(got["n_gen"], want_ngen), (got["n_gen"].tolist(), want_ngen.tolist())
    if wsp is not None:
        assert int(wsp[:64 + 4 * n_log].sum().item()) == 0  # ticket and overflow words back to zero
    return got


def _layout(mode):
    """-> (state rows, map of the logits rows)"""
    return {"batch": (3, None), "slots": (6, None), "rows": (6, [4, 1, 3])}[mode]


def _prompt(V, s, n=6):
    """A prompt of ids that no rule of these tests names (100 .. 100 + 6 n)."""
    return [100 + 7 * s + i for i in range(n)]


def _filler(s, n):
    """Generated tokens that no rule of these tests names, distinct per row."""
    return [200 + 11 * s + i for i in range(n)]


MODES = ["batch", "slots", "rows"]


# ------------------------------------------------------------------------------------------------
# 1. the ban before the minimum
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("do_sample", [0, 1], ids=["greedy", "sampling"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("V,two_stage", FORMS, ids=FORM_IDS)
def test_min_new_boundary(gpu, V, two_stage, mode, do_sample):
    """m = 3: at step m - 1 the arg-max, planted on a banned id, is not chosen (the runner-up is) and the row goes on; at step m the
    same scores choose it and the row ends.  Banned: EOS and the stop ids 0, 31, 32, V - 1."""
    from tcavt_amd.stopping import StopRules

    dev = gpu["device"]
    n_state, lrows = _layout(mode)
    eos, m = 77, 3
    rules = StopRules(V, stop_token_ids=[0, 31, 32, V - 1], min_new_tokens=m)
    banned = [31, eos, V - 1, 32, 0, 31]
    for step, ends in ((m - 1, False), (m, True)):
        specs = [_spec(_prompt(V, s), _filler(s, step), {banned[s]: TOP, 40 + s: SECOND}) for s in range(n_state)]
        got = _run(dev, mode, V, two_stage, specs, rules, eos=eos, do_sample=do_sample, lrows=lrows)
        for s, tok in got["tokens"].items():
            assert tok == (banned[s] if ends else 40 + s), (step, s, tok)
            assert int(got["finished"][s]) == int(ends)
        live_rows = [(OUT_ROWS[s] if mode != "batch" else s) for s in got["tokens"]]
        assert sorted(got["reason"][live_rows].tolist()) == (sorted(1 if banned[s] == eos else 2 for s in got["tokens"]) if ends
                                                             else [SENT] * len(live_rows))


@pytest.mark.parametrize("do_sample", [0, 1], ids=["greedy", "sampling"])
@pytest.mark.parametrize("two_stage", [False, True], ids=["one_stage", "two_stage"])
def test_min_new_ban_reaches_the_fallback_of_the_two_stage_form(gpu, two_stage, do_sample):
    """A constant row overflows every slice's candidate list, so stage 2 falls back to its own passes over the row in memory: the
    ban the slices applied must be there.  Id 0 is banned, so the first maximum (greedy) is id 1."""
    from tcavt_amd.stopping import StopRules

    dev = gpu["device"]
    V = 128256
    rules = StopRules(V, stop_token_ids=[0, 1, 5], min_new_tokens=2)
    flat = {i: 1.25 for i in range(V)}
    specs = [_spec(_prompt(V, s), _filler(s, 1), flat if s == 1 else {31: TOP}) for s in range(3)]
    got = _run(dev, "batch", V, two_stage, specs, rules, eos=3, do_sample=do_sample)
    if not do_sample:
        assert got["tokens"][1] == 2  # ids 0 and 1 are banned
    assert not got["finished"].any()


# ------------------------------------------------------------------------------------------------
# 2. stop tokens
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("V,two_stage", FORMS, ids=FORM_IDS)
def test_stop_token_ids(gpu, V, two_stage, mode):
    """Ids 31, 32 and V - 1 (a word's last bit, the next word's first, the bitmap's last) end their rows with reason 2; ids 30, 33
    and V - 2 beside them do not."""
    from tcavt_amd.stopping import StopRules

    dev = gpu["device"]
    n_state, lrows = _layout(mode)
    rules = StopRules(V, stop_token_ids=[31, 32, V - 1])
    for planted in ([31, 32, V - 1, 33, 31, 30], [33, V - 2, 30, V - 1, 32, 31]):
        specs = [_spec(_prompt(V, s), _filler(s, 4), {planted[s]: TOP}) for s in range(n_state)]
        for do_sample in (0, 1):
            got = _run(dev, mode, V, two_stage, specs, rules, eos=-1, do_sample=do_sample, lrows=lrows)
            for s, tok in got["tokens"].items():
                assert tok == planted[s] and int(got["finished"][s]) == int(tok in (31, 32, V - 1)), (s, tok)


# ------------------------------------------------------------------------------------------------
# 3. stop sequences
# ------------------------------------------------------------------------------------------------
SEQ1, SEQ3, SEQ8 = [61], [62, 63, 64], [65, 66, 67, 68, 69, 70, 71, 72]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("V,two_stage", FORMS, ids=FORM_IDS)
def test_stop_sequence_lengths(gpu, V, two_stage, mode):
    """Lengths 1, 3 and 8 fire on the token that completes them; a wrong element in the middle, or a missing first one, does not."""
    from tcavt_amd.stopping import StopRules

    dev = gpu["device"]
    n_state, lrows = _layout(mode)
    rules = StopRules(V, stop_sequences=[SEQ1, SEQ3, SEQ8])
    f = _filler
    gens = [(f(0, 7), SEQ1[0], True),                                  # length 1
            (f(1, 5) + SEQ3[:2], SEQ3[2], True),                        # length 3
            (SEQ8[:7], SEQ8[7], True),                                  # length 8, the row's first 8 tokens: step + 1 == n
            (f(3, 5) + [SEQ3[0], 99], SEQ3[2], False),                  # wrong middle
            (SEQ8[:3] + [99] + SEQ8[4:7], SEQ8[7], False),              # one wrong element of eight
            (f(5, 6) + [SEQ3[1]], SEQ3[2], False)]                      # the first element is missing
    want = {s: fires for s, (_, _, fires) in enumerate(gens)}
    specs = [_spec(_prompt(V, s), gens[s][0], {gens[s][1]: TOP}) for s in range(n_state)]
    got = _run(dev, mode, V, two_stage, specs, rules, lrows=lrows)
    for s, tok in got["tokens"].items():
        assert tok == gens[s][1] and int(got["finished"][s]) == int(want[s]), (s, tok)
        row = OUT_ROWS[s] if mode != "batch" else s
        assert int(got["reason"][row]) == (3 if want[s] else SENT) and int(got["n_gen"][row]) == (8 if want[s] else SENT)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("V,two_stage", FORMS, ids=FORM_IDS)
def test_stop_sequence_never_reaches_into_the_prompt(gpu, V, two_stage, mode):
    """The prompt ends on the head of a sequence (or holds a whole decoy occurrence): a match that would need a prompt token does
    not fire; the same tokens as the row's own first n do, at exactly step + 1 == n."""
    from tcavt_amd.stopping import StopRules

    dev = gpu["device"]
    n_state, lrows = _layout(mode)
    rules = StopRules(V, stop_sequences=[SEQ3, SEQ8])
    P = lambda s: _prompt(V, s)  # noqa: E731
    # step 0: the whole head is prompt
    heads = [SEQ3[:2], SEQ8[:7], SEQ3[:2], SEQ8[:7], SEQ3[:2], SEQ8[:7]]
    lasts = [SEQ3[2], SEQ8[7], SEQ3[2], SEQ8[7], SEQ3[2], SEQ8[7]]
    specs = [_spec(P(s) + heads[s], [], {lasts[s]: TOP}) for s in range(n_state)]
    got = _run(dev, mode, V, two_stage, specs, rules, lrows=lrows)
    assert not got["finished"].any() and all(tok == lasts[s] for s, tok in got["tokens"].items())
    # step 1: one element generated, the rest of the head in the prompt
    specs = [_spec(P(s) + heads[s][:-1], heads[s][-1:], {lasts[s]: TOP}) for s in range(n_state)]
    got = _run(dev, mode, V, two_stage, specs, rules, lrows=lrows)
    assert not got["finished"].any() and all(tok == lasts[s] for s, tok in got["tokens"].items())
    # step 2: rows 0, 2, 4 have generated SEQ3's head themselves (fires, step + 1 == 3); rows 1, 3, 5 hold all but two of SEQ8's
    # head in the prompt (does not); every prompt also holds a whole decoy occurrence of SEQ3
    specs = [_spec(P(s) + SEQ3 + heads[s][:-2], heads[s][-2:], {lasts[s]: TOP}) for s in range(n_state)]
    got = _run(dev, mode, V, two_stage, specs, rules, lrows=lrows)
    for s, tok in got["tokens"].items():
        assert tok == lasts[s] and int(got["finished"][s]) == int(s % 2 == 0), (s, tok)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("V,two_stage", FORMS, ids=FORM_IDS)
def test_bad_sequence_lengths_never_match(gpu, V, two_stage, mode):
    """Length-array entries 0 and 9 (and a negative and a huge one): those sequences never match -- although their ids, read as a
    sequence of length 1 or 8, are exactly what the rows produce -- the valid one beside them still does, and nothing faults."""
    from tcavt_amd.stopping import StopRules

    dev = gpu["device"]
    n_state, lrows = _layout(mode)
    rules = StopRules(V, stop_sequences=[SEQ1, SEQ8, SEQ3, [73], [74]])
    only_valid = StopRules(V, stop_sequences=[SEQ3])
    f = _filler
    gens = [(f(0, 7), SEQ1[0]), (SEQ8[:7], SEQ8[7]), (f(2, 5) + SEQ3[:2], SEQ3[2]), (f(3, 7), 73), (f(4, 7), 74), (SEQ8[:7], SEQ8[7])]
    specs = [_spec(_prompt(V, s), gens[s][0], {gens[s][1]: TOP}) for s in range(n_state)]
    got = _run(dev, mode, V, two_stage, specs, rules, lrows=lrows, expect_rules=only_valid, seq_len=[0, 9, 3, -1, 1 << 30])
    for s, tok in got["tokens"].items():
        assert tok == gens[s][1] and int(got["finished"][s]) == int(s == 2), (s, tok)


# ------------------------------------------------------------------------------------------------
# 4. precedence, finished rows, pad rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("V,two_stage", FORMS, ids=FORM_IDS)
def test_precedence_of_the_reasons(gpu, V, two_stage, mode):
    """EOS that is also a stop token and a one-token sequence: reason 1.  A stop token that also completes a sequence: 2.  In the
    slots and rows forms, on the budget's last step: a stop token gives 2, a sequence 3, nothing else 4."""
    from tcavt_amd.stopping import StopRules

    dev = gpu["device"]
    n_state, lrows = _layout(mode)
    eos = 55
    rules = StopRules(V, stop_token_ids=[eos, 32], stop_sequences=[[eos], [31, 32], SEQ3])
    f = _filler
    B = 5  # step + 1 of every row below
    cases = [(f(0, 4), eos, 1 << 20, 1), (f(1, 3) + [31], 32, 1 << 20, 2), (f(2, 2) + SEQ3[:2], SEQ3[2], 1 << 20, 3),
             (f(3, 4), 32, B, 2), (f(4, 2) + SEQ3[:2], SEQ3[2], B, 3), (f(5, 4), 90, B, 4)]
    specs = [_spec(_prompt(V, s), cases[s][0], {cases[s][1]: TOP}, budget=cases[s][2]) for s in range(n_state)]
    got = _run(dev, mode, V, two_stage, specs, rules, eos=eos, lrows=lrows)
    for s, tok in got["tokens"].items():
        row = OUT_ROWS[s] if mode != "batch" else s
        assert tok == cases[s][1] and int(got["reason"][row]) == cases[s][3] and int(got["n_gen"][row]) == B, (s, tok)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("V,two_stage", FORMS, ids=FORM_IDS)
def test_finished_rows_and_pad_rows_write_no_record(gpu, V, two_stage, mode):
    """A finished row: cur_tok becomes pad and the two records keep their sentinels (slots / rows: nothing else is written either),
    although its scores would end it again; rows form: map entries -1 and S write nothing at all."""
    from tcavt_amd.stopping import StopRules

    dev = gpu["device"]
    n_state, lrows = _layout(mode)
    if mode == "rows":
        lrows = [-1, n_state, 2]
    rules = StopRules(V, stop_token_ids=[31], stop_sequences=[SEQ1], min_new_tokens=1)
    specs = [_spec(_prompt(V, s), _filler(s, 3), {31: TOP}, fin=int(s in (0, 2))) for s in range(n_state)]
    got = _run(dev, mode, V, two_stage, specs, rules, eos=4, lrows=lrows)
    live = {"batch": [1], "slots": [1, 3, 4, 5], "rows": []}[mode]
    assert sorted(got["tokens"]) == live and all(t == 31 for t in got["tokens"].values())
    assert int((got["reason"] != SENT).sum()) == len(live) == int((got["n_gen"] != SENT).sum())


# ------------------------------------------------------------------------------------------------
# 5. no rules: the existing entries, array for array
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("V,two_stage", FORMS, ids=FORM_IDS)
def test_no_rules_equals_the_existing_entry(gpu, V, two_stage, mode):
    """tcavt_sample_tokens with stop = NULL, and with a struct in which nothing is set, against the existing entry of the form: every
    output array, the logits in place and the workspace's control words (zero)."""
    from tcavt_amd import capi, ops

    dev = gpu["device"]
    i32, i64 = torch.int32, torch.int64
    n_state, lrows = _layout(mode)
    n_log = len(lrows) if lrows is not None else n_state
    slots = mode != "batch"
    g = torch.Generator().manual_seed(7)
    hist0 = torch.randint(0, min(V, 300), (n_state, 40), generator=g)
    hist0[:, 30:] = 0
    hist0[0, :30] = torch.arange(30) % 7 + 8  # repeats: the n-gram ban and the penalty have work to do
    base = torch.from_numpy(_base(V)[:n_log])
    for do_sample in (1, 0):
        params = capi.SampleParams(0.9, 0.9, 1.2, 40, 3, do_sample, int(base[0].argmax()), PAD, 1234)  # row 0 may end on EOS
        res = []
        for entry in ("old", "null", "empty"):
            logits = base.clone().to(dev)
            st = dict(history=hist0.clone().to(dev), hist_len=torch.full((n_state,), 30, dtype=i32, device=dev),
                      step=torch.full((n_state if slots else 1,), 3, dtype=i32, device=dev), cur=torch.zeros(n_state, dtype=i64, device=dev),
                      pos=torch.full((n_state,), 50, dtype=i32, device=dev), finished=torch.zeros(n_state, dtype=i32, device=dev),
                      out=torch.full((10 if slots else n_state, 8), OUT_SENT, dtype=i64, device=dev))
            st["finished"][n_state - 1] = 1
            max_new = torch.tensor([1 << 20, 5, 4, 9, 5, 7][:n_state], dtype=i32, device=dev) if slots else None
            out_row = torch.tensor(OUT_ROWS[:n_state], dtype=i64, device=dev) if slots else None
            sor = torch.tensor(lrows, dtype=i32, device=dev) if mode == "rows" else None
            wsp = ops.sample_workspace(n_log, dev) if two_stage else None
            for _ in range(2):
                if entry == "old":
                    if mode == "batch":
                        ops.sample_logits(logits, st["history"], st["hist_len"], params, st["step"], st["cur"], st["pos"], st["finished"],
                                          st["out"], advance_pos=True, workspace=wsp)
                    elif mode == "slots":
                        ops.sample_logits_slots(logits, st["history"], st["hist_len"], params, st["step"], max_new, out_row, st["cur"],
                                                st["pos"], st["finished"], st["out"], advance_pos=True, workspace=wsp)
                    else:
                        ops.sample_logits_rows(logits, sor, st["history"], st["hist_len"], params, st["step"], max_new, out_row, st["cur"],
                                               st["pos"], st["finished"], st["out"], advance_pos=True, workspace=wsp)
                else:
                    ops.sample_tokens(logits, st["history"], st["hist_len"], params, st["step"], st["cur"], st["pos"], st["finished"],
                                      st["out"], advance_pos=True, workspace=wsp, max_new=max_new, out_row=out_row, slot_of_row=sor,
                                      stop=capi.StopRules() if entry == "empty" else None)
            torch.cuda.synchronize()
            if wsp is not None:
                assert int(wsp[:64 + 4 * n_log].sum().item()) == 0
            res.append([logits.cpu()] + [st[k].cpu() for k in ("history", "hist_len", "step", "cur", "pos", "finished", "out")])
        for other in res[1:]:
            assert torch.equal(torch.isinf(res[0][0]), torch.isinf(other[0]))
            assert torch.equal(torch.nan_to_num(res[0][0], neginf=0.0), torch.nan_to_num(other[0], neginf=0.0))
            for x, y, nm in zip(res[0][1:], other[1:], ("history", "hist_len", "step", "cur", "pos", "finished", "out")):
                assert torch.equal(x, y), (nm, do_sample)
        assert int((res[0][7] != OUT_SENT).sum()) > 0


# ------------------------------------------------------------------------------------------------
# 6. the model: a run with rules is the unruled run, cut
# ------------------------------------------------------------------------------------------------
_MODEL = {}


def _setup(dev):
    """The fixture model, built once for the module."""
    if "m" not in _MODEL:
        from tcavt_amd import model

        fx, cfg, weights, t = load_generation_case()
        m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights, device=dev).eval()
        _MODEL.update(m=m, fx=fx, cfg=cfg, weights=weights, t=t, g={k: v.to(dev) for k, v in t.items()})
    return _MODEL


def _batch(M, **kw):
    g = M["g"]
    res = M["m"].mllm.generate_batch(g["vision_emb"], None, input_ids=g["input_ids"], attention_mask=g["attention_mask"], **kw)
    torch.cuda.synchronize()
    M["m"].mllm.check_flags()
    return res


def _first_new(row, k0, width=1):
    """The first step k >= k0 at which row[k : k + width] holds only tokens the row has not produced before step k."""
    for k in range(k0, len(row) - width + 1):
        if not set(row[k:k + width]) & set(row[:k]) and len(set(row[k:k + width])) == width:
            return k
    raise AssertionError(f"no step >= {k0} of {row} has tokens new to the row: the fixture changed, choose other steps")


def _rules_from(rows, V, tok_row, tok_k0, seq_row, seq_k0, extra_tokens=()):
    """Rules that must fire on the unruled rows: a stop token = what row `tok_row` emitted at (the first new step >=) tok_k0, and a
    3-token sequence = row `seq_row`'s steps seq_k0 .. seq_k0 + 2 (likewise)."""
    from tcavt_amd.stopping import StopRules

    kt = _first_new(rows[tok_row], tok_k0)
    ks = _first_new(rows[seq_row], seq_k0, 3)
    return StopRules(V, stop_token_ids=[rows[tok_row][kt], *extra_tokens], stop_sequences=[rows[seq_row][ks:ks + 3]])


@pytest.mark.parametrize("do_sample", [True, False], ids=["sampling", "greedy"])
def test_generate_batch_with_rules_is_the_unruled_run_cut(gpu, do_sample):
    """Rules built from an unruled run's own tokens: row 0's step-5 token as a stop token, row 1's steps 7 .. 9 as a sequence, row 2
    left to run out.  poll_every None / 1 / 4, eager and hipGraph: the same rows, records as first_end says.
    The batch form has no device budget, so a row that runs out never sets its flag and the polled loop cannot leave early while
    one does: with row 2 running out, steps == max_new_tokens - 1 with or without polling.  The early exit is therefore checked
    with one more stop token that ends row 2 as well: then the polled runs take fewer steps than the unpolled one, and the same
    rows come out."""
    M = _setup(gpu["device"])
    V, N = M["cfg"].llama.vocab, 16
    kw = dict(max_new_tokens=N, do_sample=do_sample, seed=21, pad_token_id=PAD)
    plain = _batch(M, **kw).cpu()
    rows = plain.tolist()
    rules = _rules_from(rows, V, 0, 5, 1, 7)
    want = [cut_row(rules, r, None, PAD) for r in rows]
    reasons = [w[2] for w in want]
    assert len({r for r in reasons if r != 4}) >= 2 and 4 in reasons, reasons  # two rules fire, and one row runs out
    rk = dict(stop_token_ids=rules.stop_token_ids, stop_sequences=rules.stop_sequences, return_info=True)
    for use_graph in (False, True):
        for poll in (None, 1, 4):
            out, info = _batch(M, use_graph=use_graph, poll_every=poll, **kw, **rk)
            assert out.cpu().tolist() == [w[0] for w in want], (use_graph, poll)
            assert info["finish_reason"].dtype == info["n_generated"].dtype == torch.int32
            assert info["finish_reason"].tolist() == reasons and info["n_generated"].tolist() == [w[1] for w in want]
            assert info["steps"] == N - 1  # (a row runs out: see the docstring)
    # every row ends: the polled loop leaves early
    last = _first_new(rows[2], 3)
    rules2 = _rules_from(rows, V, 0, 5, 1, 7, extra_tokens=[rows[2][last]])
    want2 = [cut_row(rules2, r, None, PAD) for r in rows]
    n_max = max(w[1] for w in want2)
    assert 4 not in [w[2] for w in want2] and n_max < N - 4
    rk2 = dict(stop_token_ids=rules2.stop_token_ids, stop_sequences=rules2.stop_sequences, return_info=True)
    for use_graph in (False, True):
        out0, info0 = _batch(M, use_graph=use_graph, **kw, **rk2)
        assert info0["steps"] == N - 1 and out0.cpu().tolist() == [w[0] for w in want2]
        for poll in (1, 4):
            out, info = _batch(M, use_graph=use_graph, poll_every=poll, **kw, **rk2)
            assert torch.equal(out, out0) and info["finish_reason"].tolist() == [w[2] for w in want2]
            assert info["n_generated"].tolist() == [w[1] for w in want2]
            # the last row's ending token comes out of step n_max - 1; the loop sees it at the next multiple of poll_every
            assert n_max - 1 <= info["steps"] <= n_max - 1 + poll - 1 < N - 1, (poll, info["steps"])


IDX = [0, 1, 2, 0, 1, 2, 0, 1, 2, 0]  # ten requests: the fixture's three, each on its own Philox row


def _pool(M, **kw):
    g = M["g"]
    i = torch.tensor(IDX, device=g["input_ids"].device)
    res = M["m"].mllm.generate_pool(g["vision_emb"][i], g["input_ids"][i], g["attention_mask"][i], **kw)
    torch.cuda.synchronize()
    M["m"].mllm.check_flags()
    return res


def _pool_rules(rows, V, N):
    """Rules from the unruled rows that fire as the test needs -- decided by first_end on those rows alone: a stop token = request
    0's token at a step >= 5 that ends request 0 there, a 3-token sequence = three consecutive steps >= 7 of request 1 that end
    request 1 there (so neither stop token may occur in it earlier), the FIRST token of some other request q0 as a second stop token,
    and at least one request left to run out.  The ten requests share three prompts, so tokens recur between them: the first
    combination that satisfies all four is taken.  -> (rules, q0)"""
    from tcavt_amd.stopping import StopRules

    for kt in range(5, N):
        for ks in range(7, N - 2):
            for q0 in range(2, len(rows)):
                rules = StopRules(V, stop_token_ids=[rows[0][kt], rows[q0][0]], stop_sequences=[rows[1][ks:ks + 3]])
                ends = [rules.first_end(r, None, budget=N) for r in rows]
                if ends[0] == (kt + 1, 2) and ends[1] == (ks + 3, 3) and ends[q0] == (1, 2) and any(e[1] == 4 for e in ends):
                    return rules, q0
    raise AssertionError(f"no rule set from these rows fires as needed: the fixture changed\n{rows}")


@pytest.mark.parametrize("G", [1, 2], ids=["admit1", "admit2"])
def test_generate_pool_with_rules_is_the_unruled_run_cut(gpu, G):
    """Ten requests on three slots, sampling: rules from the unruled pool run's own tokens (a token of request 0 at a step >= 5,
    three steps >= 7 of request 1, and some request's FIRST token, which ends it at its admission: _pool_rules).  Every request's row is its unruled row cut, its
    records are first_end's, the result does not depend on the number of slots or on eager / hipGraph, and fewer steps are run."""
    M = _setup(gpu["device"])
    mm = M["m"].mllm
    V, N = M["cfg"].llama.vocab, 12
    kw = dict(max_new_tokens=N, slots=3, admit_group=G, do_sample=True, seed=33, pad_token_id=PAD)
    plain = _pool(M, **kw).cpu()
    steps_plain = mm.pool_stats["steps"]
    assert "finish_reason" not in mm.pool_stats
    rows = plain.tolist()
    rules, q0 = _pool_rules(rows, V, N)
    want = [cut_row(rules, r, None, PAD, budget=N) for r in rows]
    reasons = [w[2] for w in want]
    assert len({r for r in reasons if r != 4}) >= 2 and 4 in reasons and want[q0][1] == 1, reasons
    rk = dict(stop_token_ids=rules.stop_token_ids, stop_sequences=rules.stop_sequences)
    outs = []
    for slots, use_graph in ((3, True), (3, False), (5, True)):
        out, stats = _pool(M, **{**kw, "slots": slots}, use_graph=use_graph, return_info=True, **rk)
        assert stats is mm.pool_stats
        assert out.cpu().tolist() == [w[0] for w in want], (slots, use_graph)
        assert stats["finish_reason"].tolist() == reasons and stats["n_generated"].tolist() == [w[1] for w in want]
        assert stats["finish_reason"].dtype == stats["n_generated"].dtype == torch.int32
        if slots == 3:
            assert stats["steps"] < steps_plain, (stats["steps"], steps_plain)
        assert sorted(r for r, _, _ in stats["admitted"]) == list(range(10))
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_min_new_tokens_through_the_whole_stack(gpu):
    """min_new_tokens = 4 with the unruled greedy token of row 0's step 1 in the stop set: the ban changes that token, and
    generate_batch and generate_pool (admit_group = 1) give the same rows."""
    M = _setup(gpu["device"])
    g, V, N = M["g"], M["cfg"].llama.vocab, 10
    kw = dict(max_new_tokens=N, do_sample=False, pad_token_id=PAD)
    plain = _batch(M, **kw).cpu()
    stop = int(plain[0, 1])
    rk = dict(stop_token_ids=[stop], min_new_tokens=4)
    a, info = _batch(M, return_info=True, **kw, **rk)
    b = M["m"].mllm.generate_pool(g["vision_emb"], g["input_ids"], g["attention_mask"], slots=3, admit_group=1, **kw, **rk)
    torch.cuda.synchronize()
    M["m"].mllm.check_flags()
    stats = M["m"].mllm.pool_stats
    assert torch.equal(a, b)
    assert int(a[0, 0]) == int(plain[0, 0]) and int(a[0, 1]) != stop  # the ban is exercised
    assert stop not in a[:, :4].reshape(-1).tolist()
    assert info["finish_reason"].tolist() == stats["finish_reason"].tolist() and info["n_generated"].tolist() == stats["n_generated"].tolist()
    from tcavt_amd.stopping import StopRules

    rules = StopRules(V, stop_token_ids=[stop])
    for r in range(3):  # what came out obeys the rules it was generated under
        n, reason = rules.first_end(a[r].tolist()[:int(info["n_generated"][r])], None, budget=N)
        assert (n, reason) == (int(info["n_generated"][r]), int(info["finish_reason"][r])) and n >= 4
        assert (a[r, n:] == PAD).all()


def test_defaults_are_untouched(gpu):
    """Without any new argument both entries return a tensor, equal to a call that passes empty rules explicitly."""
    M = _setup(gpu["device"])
    mm = M["m"].mllm
    empty = dict(stop_token_ids=None, stop_sequences=None, min_new_tokens=0, return_info=False)
    empty2 = dict(stop_token_ids=[], stop_sequences=[], min_new_tokens=0, return_info=False)
    kw = dict(max_new_tokens=8, do_sample=True, seed=4)
    a = _batch(M, **kw)
    assert isinstance(a, torch.Tensor)
    assert torch.equal(a, _batch(M, poll_every=None, **kw, **empty)) and torch.equal(a, _batch(M, **kw, **empty2))
    out, info = _batch(M, return_info=True, **kw)  # the records alone change no token
    assert torch.equal(a, out) and info["finish_reason"].tolist() == [4] * 3 and info["n_generated"].tolist() == [8] * 3 and info["steps"] == 7
    pk = dict(max_new_tokens=[8, 5, 8, 3, 8, 8, 8, 2, 8, 8], slots=3, do_sample=True, seed=4)
    p = _pool(M, **pk)
    assert isinstance(p, torch.Tensor) and "finish_reason" not in mm.pool_stats
    assert torch.equal(p, _pool(M, **pk, **empty)) and torch.equal(p, _pool(M, **pk, **empty2))
    out, stats = _pool(M, return_info=True, **pk)
    assert torch.equal(p, out) and stats["finish_reason"].tolist() == [4] * 10 and stats["n_generated"].tolist() == pk["max_new_tokens"]
