"""tcavt_spec_verify against sequential ops.sample_tokens calls on the same logits rows: exact, greedy and sampled.

The logits are the test's: fp32 [S * T, V] random (3 * N(0, 1)); the two ending tokens sit 60 below that everywhere but where an
event is wanted, and 60 above it there: selected, or not, whatever the warpers do.  V = 512 and 4100, k = 1, 3, 7 (T = k + 1); repetition penalty 1.2 and no-repeat-3-gram throughout; greedy and three
sampled settings (temperature, top_k, top_p) = (0.9, 40, 0.9) -- the reference's defaults --, (0.7, 5, 1.0), (1.3, 200, 0.5); EOS =
V - 1, stop set {V - 2}, min_new_tokens = 5; out_row a permutation of the sequences (the Philox row and the row of the records).

Reference ("the plain loop"): per sequence s and offset j = 0, 1, .. one ops.sample_tokens call in its slots form on the one-row view
logits[s * T + j] and one-entry views of the state of s -- the call a plain decode step would make for that token --, continued while
j < n_draft[s], the selected token equals draft j and the row has not ended.  A first pass of it with every draft "right" yields the
tokens the sampler would choose; the drafts of the real run are made from them: sequence a in 0 .. k gets a right drafts and a wrong
one behind them (accepted length a: every value 0 .. k), one of them with fewer than k drafts, and five special sequences:
  - the draft that equals EOS: right drafts up to an EOS spike -- the EOS is committed as the model's token, not counted as accepted;
  - a stop-set token at offset 1 (finish reason 2);
  - min_new_tokens falling inside the block: EOS spikes in every row, banned while step < 5, so the row ends exactly at step 5;
  - the budget ending inside the block (max_new = step + 2: finish reason 4 at offset 1);
  - a sequence that is finished on entry (inert: cur_tok = pad, nothing else written).
Asserted: out, history, hist_len, pos, step, cur, finished, finish_reason and n_generated equal the reference's, the drafted and
accepted counters equal the reference loop's counts (on top of a non-zero start: they accumulate), and from the reference alone that
every event above happened.  The scratch and the counters live between sentinel bands."""
import pytest
import torch

pytestmark = pytest.mark.gpu

I32, I64, F32 = torch.int32, torch.int64, torch.float32
PAD, CAP, N_OUT, MIN_NEW, STEP0, BAND = 3, 64, 48, 5, 9, 8
PARAMS = {"greedy": (False, 1.0, 1, 1.0), "s_default": (True, 0.9, 40, 0.9), "s_k5": (True, 0.7, 5, 1.0), "s_p05": (True, 1.3, 200, 0.5)}


def _sp(name, V):
    from tcavt_amd import generation

    do_sample, t, k, p = PARAMS[name]
    return generation.sample_params(t, p, 1.2, k, 3, do_sample, V - 1, PAD, seed=1234)


def _state(S, V, k, dev, seed):
    """the S sequences' state before the step (CPU tensors) and the roles of the special sequences"""
    g = torch.Generator().manual_seed(seed)
    T = k + 1
    n_plain = k + 1
    roles = ["plain"] * n_plain + ["eos", "stop", "min_new", "budget", "finished"]
    assert len(roles) == S
    hist = torch.zeros(S, CAP, dtype=I64)
    hist_len = torch.zeros(S, dtype=I32)
    for s in range(S):
        L = 10 + (s * 3) % 7
        hist[s, :L] = torch.randint(4, V - 2, (L,), generator=g)  # (never EOS, the stop token or the pad id)
        hist_len[s] = L
    step = torch.full((S,), STEP0, dtype=I32)
    max_new = torch.full((S,), 40, dtype=I32)
    finished = torch.zeros(S, dtype=I32)
    jm = min(2, k)  # offset at which the minimum is reached
    step[roles.index("min_new")] = MIN_NEW - jm
    max_new[roles.index("budget")] = STEP0 + 2
    finished[roles.index("finished")] = 1
    out_row = torch.randperm(S, generator=g).to(I64)
    cur = hist[torch.arange(S), hist_len.long() - 1].clone()
    pos = (hist_len + 16).to(I32)
    logits = torch.randn(S * T, V, generator=g) * 3
    logits[:, V - 2:] -= 60.0                             # no ending token by chance
    e = roles.index("eos")
    logits[e * T + min(1, k - 1), V - 1] += 120.0         # the draft that equals EOS
    logits[roles.index("stop") * T + 1, V - 2] += 120.0   # a stop-set token at offset 1
    mn = roles.index("min_new")
    logits[mn * T:(mn + 1) * T, V - 1] += 120.0           # EOS wanted everywhere: banned below the minimum
    return dict(history=hist, hist_len=hist_len, step=step, max_new=max_new, out_row=out_row, cur=cur, pos=pos, finished=finished), logits, roles


def _dev(st, dev):
    return {k_: v.clone().to(dev) for k_, v in st.items()}


def _rules(V, S, dev):
    from tcavt_amd.stopping import StopRules

    return StopRules(V, [V - 2], None, MIN_NEW).to(dev).records(S, dev)


def _reference(st0, logits0, n_draft, drafts, sp, V, T, dev):
    """the plain loop, per sequence: -> (state, out, rules records, drafted [S], accepted [S], tokens per sequence)"""
    from tcavt_amd import ops

    S = len(n_draft)
    st = _dev(st0, dev)
    logits = logits0.clone().to(dev)
    out = torch.full((S, N_OUT), PAD, dtype=I64, device=dev)
    dr = _rules(V, S, dev)
    ws1 = ops.sample_workspace(1, dev)
    drafted, accepted, toks = [0] * S, [0] * S, [[] for _ in range(S)]
    for s in range(S):
        v = lambda name: st[name][s:s + 1]
        if not int(st["finished"][s]):
            drafted[s] = int(n_draft[s])
        for j in range(T):
            r = s * T + j
            was_finished = int(st["finished"][s])
            ops.sample_tokens(logits[r:r + 1], v("history"), v("hist_len"), sp, v("step"), v("cur"), v("pos"), v("finished"), out,
                              advance_pos=True, workspace=ws1, max_new=v("max_new"), out_row=v("out_row"), stop=dr)
            torch.cuda.synchronize()
            tok = int(st["cur"][s])
            if not was_finished:
                toks[s].append(tok)
            if int(st["finished"][s]) or j >= int(n_draft[s]) or tok != int(drafts[s][j]):
                break
            accepted[s] += 1
    return st, out, dr, drafted, accepted, toks


def _device(st0, logits0, n_draft, drafts, sp, V, T, dev, two_stage, start):
    from tcavt_amd import ops

    S, k = len(n_draft), T - 1
    R = S * T
    st = _dev(st0, dev)
    logits = logits0.clone().to(dev)
    out = torch.full((S, N_OUT), PAD, dtype=I64, device=dev)
    dr = _rules(V, S, dev)
    cur_rows = torch.full((S, T), PAD, dtype=I64)
    cur_rows[:, 0] = st0["cur"]
    for s in range(S):
        cur_rows[s, 1:1 + int(n_draft[s])] = torch.tensor(drafts[s][:int(n_draft[s])], dtype=I64)
    sbuf = torch.full((R + S + 2 * BAND,), -99, dtype=I32, device=dev)
    cbuf = torch.full((2, S + 2 * BAND), -99, dtype=I32, device=dev)
    drafted, accepted = cbuf[0, BAND:BAND + S], cbuf[1, BAND:BAND + S]
    drafted.fill_(start)
    accepted.fill_(2 * start)
    nd = torch.tensor(n_draft, dtype=I32, device=dev)
    cr = cur_rows.reshape(-1).to(dev)
    keep = (nd.clone(), cr.clone())
    a = ops.spec_verify_args(logits, T, nd, cr, sbuf[BAND:BAND + R + S], drafted, accepted, st["history"], st["hist_len"], sp, st["step"],
                             st["max_new"], st["out_row"], st["cur"], st["pos"], st["finished"], out, advance_pos=True,
                             workspace=ops.sample_workspace(R, dev) if two_stage else None, stop=dr)
    ops.spec_verify(a)
    torch.cuda.synchronize()
    assert torch.equal(nd, keep[0]) and torch.equal(cr, keep[1]), "n_draft / cur_rows modified"
    assert bool((sbuf[:BAND] == -99).all()) and bool((sbuf[-BAND:] == -99).all()), "write outside the scratch"
    assert bool((cbuf[:, :BAND] == -99).all()) and bool((cbuf[:, -BAND:] == -99).all()), "write outside the counters"
    return st, out, dr, (drafted - start).tolist(), (accepted - 2 * start).tolist()


def _run(dev, V, k, pname, two_stage=True):
    T, S = k + 1, k + 1 + 5
    sp = _sp(pname, V)
    st0, logits0, roles = _state(S, V, k, dev, seed=V + 17 * k)
    # pass 1: every draft right -> the tokens the sampler would choose at every offset
    from tcavt_amd import ops

    probe_st = _dev(st0, dev)
    probe_logits = logits0.clone().to(dev)
    probe_out = torch.full((S, N_OUT), PAD, dtype=I64, device=dev)
    dr = _rules(V, S, dev)
    ws1 = ops.sample_workspace(1, dev)
    chosen = [[] for _ in range(S)]
    for s in range(S):
        v = lambda name: probe_st[name][s:s + 1]
        for j in range(T):
            if int(probe_st["finished"][s]):
                break
            ops.sample_tokens(probe_logits[s * T + j:s * T + j + 1], v("history"), v("hist_len"), sp, v("step"), v("cur"), v("pos"), v("finished"),
                              probe_out, advance_pos=True, workspace=ws1, max_new=v("max_new"), out_row=v("out_row"), stop=dr)
            torch.cuda.synchronize()
            chosen[s].append(int(probe_st["cur"][s]))
    # the drafts of the real run
    n_draft, drafts = [], []
    for s, role in enumerate(roles):
        right = chosen[s][:k] + [4] * (k - len(chosen[s][:k]))
        if role == "plain":
            a = s  # accepted length wanted: 0 .. k
            d = right[:a] + [(t + 1) % (V - 2) if (t + 1) % (V - 2) >= 4 else 4 for t in right[a:]]
            n = k if s != 1 or k == 1 else k - 1  # one sequence drafts fewer than k ids
            d = d[:n] + [PAD] * (k - n)
            n_draft.append(n)
            drafts.append(d)
        else:
            n_draft.append(0 if role == "finished" else k)
            drafts.append(right)
    ref = _reference(st0, logits0, n_draft, drafts, sp, V, T, dev)
    got = _device(st0, logits0, n_draft, drafts, sp, V, T, dev, two_stage, start=5)
    what = f"V={V} k={k} {pname}"
    # ---- from the reference alone: the events happened
    r_st, r_out, r_dr, r_drafted, r_accepted, r_toks = ref
    assert r_accepted[:k + 1] == list(range(k + 1)), (what, r_accepted)  # every accepted length 0 .. k
    assert r_drafted == n_draft and min(n_draft[:k + 1]) == (k - 1 if k > 1 else k)
    reason = r_dr.finish_reason.cpu()[st0["out_row"]].tolist()
    n_gen = r_dr.n_generated.cpu()[st0["out_row"]].tolist()
    e, stp, mn, bd, fn = (roles.index(x) for x in ("eos", "stop", "min_new", "budget", "finished"))
    je = min(1, k - 1)
    assert reason[e] == 1 and r_toks[e][-1] == V - 1 and len(r_toks[e]) == je + 1 and r_accepted[e] == je, (what, r_toks[e], r_accepted[e])
    assert drafts[e][je] == V - 1  # the draft did equal EOS: committed as the model's token, not counted
    assert reason[stp] == 2 and r_toks[stp][-1] == V - 2 and len(r_toks[stp]) == 2, (what, r_toks[stp])
    assert reason[mn] == 1 and n_gen[mn] == MIN_NEW + 1 and V - 1 not in r_toks[mn][:-1] and r_accepted[mn] == min(2, k), (what, r_toks[mn], n_gen[mn])
    assert reason[bd] == 4 and len(r_toks[bd]) == 2 and n_gen[bd] == STEP0 + 2, (what, r_toks[bd])
    assert r_toks[fn] == [] and r_drafted[fn] == 0 and int(r_st["cur"][fn]) == PAD
    for s in range(k + 1):
        assert len(r_toks[s]) == r_accepted[s] + 1, (what, s)
    # ---- the device run equals it
    g_st, g_out, g_dr, g_drafted, g_accepted = got
    for name in ("history", "hist_len", "pos", "step", "cur", "finished", "max_new", "out_row"):
        assert torch.equal(g_st[name], r_st[name]), f"{what}: {name}: {g_st[name].tolist()} != {r_st[name].tolist()}"
    assert torch.equal(g_out, r_out), f"{what}: out"
    assert torch.equal(g_dr.finish_reason, r_dr.finish_reason) and torch.equal(g_dr.n_generated, r_dr.n_generated), f"{what}: records"
    assert g_drafted == r_drafted and g_accepted == r_accepted, f"{what}: counters {g_drafted} {g_accepted} != {r_drafted} {r_accepted}"


@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("V", [512, 4100])
def test_commit_equals_sequential_sampler_calls(gpu, V, k, pname):
    _run(gpu["device"], V, k, pname)


@pytest.mark.parametrize("pname", ["greedy", "s_default"])
def test_one_stage_form(gpu, pname):
    """without a workspace the sampler runs its one-workgroup form: the same commit"""
    _run(gpu["device"], 512, 3, pname, two_stage=False)
