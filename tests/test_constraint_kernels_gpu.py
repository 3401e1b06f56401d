"""tcavt_constraint_build / _mask / _advance against the host statement of the rule (constraint.TokenConstraint.allowed / next),
with exact equality: the scores of allowed tokens keep their bits, the others are -inf, the states are equal.  Shapes: the
decoder's vocabulary and one that is no multiple of 128 (the tail word, the tail group of four); 1, 8 and 32 rows; the batch,
slots and rows forms.  The automaton has a state that allows everything, one that allows token 0 only, one that allows token
V - 1 only, one that allows one token on each side of two bitmap word boundaries, and a mixed one."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VOCABS = (128256, 1000)
ROWS = (1, 8, 32)
I32, I64 = torch.int32, torch.int64
FREE, ONLY_FIRST, ONLY_LAST, BOUNDARY, MIXED = range(5)
_CACHE = {}


def _constraint(V):
    """-> (TokenConstraint, allowed bool [5, V], scores fp32 [32, V]), made once per vocabulary and never changed."""
    if V not in _CACHE:
        from tcavt_amd.constraint import TokenConstraint

        token_class = torch.zeros(V, dtype=I32)
        token_class[5::7] = 4  # a class spread over every word: the mixed state bans it inside otherwise allowed groups
        token_class[0], token_class[V - 1] = 1, 2
        token_class[[31, 32, 63, 64]] = 3
        trans = torch.tensor([[0, 1, 2, 3, 4],        # FREE: everything, and every class leads somewhere else
                              [-1, 2, -1, -1, -1],    # ONLY_FIRST: token 0
                              [-1, -1, 3, -1, -1],    # ONLY_LAST: token V - 1
                              [-1, -1, -1, 4, -1],    # BOUNDARY: 31, 32, 63, 64
                              [4, -1, 0, 1, -1]],     # MIXED: everything but token 0 and class 4
                             dtype=I32)
        C = TokenConstraint(token_class, trans)
        allowed = np.zeros((5, V), dtype=bool)
        for s in range(5):
            allowed[s, C.allowed(s)] = True
        g = np.random.default_rng(4242 + V)
        x = (g.standard_normal((32, V)) * 3.0).astype(np.float32)
        x[:, 17] = -np.inf  # a score that is banned already
        x[1, 3] = np.float32("nan")  # bits are bits
        _CACHE[V] = (C, allowed, x)
    return _CACHE[V]


def test_build_makes_the_bitmaps_and_counts_of_the_host_rule(gpu):
    from tcavt_amd import ops

    for V in VOCABS:
        C, allowed, _ = _constraint(V)
        T = ops.ConstraintTable(C.token_class, C.trans, gpu["device"]).build()
        torch.cuda.synchronize()
        words = T.bitmap.cpu().numpy().view(np.uint32)
        assert words.shape == (5, (V + 31) // 32)
        bits = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(5, -1)
        assert np.array_equal(bits[:, :V], allowed) and not bits[:, V:].any()
        assert T.count.cpu().tolist() == allowed.sum(1).tolist() == [V, 1, 1, 4, int(allowed[MIXED].sum())]


def _scene(V, R, form, dev):
    """The state of one call: -> dict of device tensors plus the host expectation per logits row (live, slot, request, state)."""
    g = np.random.default_rng(R * 131 + V + len(form))
    n_state = R if form != "rows" else R + 3
    n_req = n_state + 2
    d = dict(n_state=n_state, n_req=n_req)
    if form == "batch":
        slot_of_row, out_row = None, None
        request = np.arange(n_state)
    else:
        request = g.permutation(n_req)[:n_state]
        out_row = torch.from_numpy(request.astype(np.int64)).to(dev)
        slot_of_row = None
        if form == "rows":
            m = g.permutation(n_state)[:R].astype(np.int32)
            if R > 1:
                m[R // 2] = -1  # a pad row of a grouped admission
            slot_of_row = torch.from_numpy(m).to(dev)
    finished = np.zeros(n_state, dtype=np.int32)
    if R > 1:
        finished[g.permutation(n_state)[:max(1, n_state // 4)]] = 1
    start = g.integers(0, 5, n_req).astype(np.int32)
    stale = g.integers(0, 5, n_state).astype(np.int32)
    d.update(slot_of_row=slot_of_row, out_row=out_row, finished=torch.from_numpy(finished).to(dev), start=torch.from_numpy(start).to(dev),
             request=request, finished_host=finished, start_host=start, stale=stale)
    return d


def _expect(d, form, R, step_host):
    """Per logits row: None (inert / skipped) or (slot, request, state the mask must use)."""
    rows = []
    m = d["slot_of_row"].cpu().numpy() if d["slot_of_row"] is not None else np.arange(R)
    for r in range(R):
        s = int(m[r])
        if s < 0 or d["finished_host"][s]:
            rows.append(None)
            continue
        q = int(d["request"][s])
        step = int(step_host[s] if form != "batch" else step_host[0])
        rows.append((s, q, int(d["start_host"][q]) if step == 0 else int(d["stale"][s])))
    return rows


@pytest.mark.parametrize("form", ["batch", "slots", "rows"])
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("V", VOCABS)
def test_mask_and_advance_equal_the_host_rule(gpu, V, R, form):
    from tcavt_amd import ops

    dev = gpu["device"]
    C, allowed, x = _constraint(V)
    T = ops.ConstraintTable(C.token_class, C.trans, dev).build()
    d = _scene(V, R, form, dev)
    n_state = d["n_state"]
    ws = torch.empty(ops.constraint_workspace_bytes(R), dtype=torch.uint8, device=dev)
    # the batch form has one step word: one call at step 0 (every row takes start[r], whatever its state word holds) and one at
    # step 3 (every row takes its state word); the slot forms mix the two in one call
    step_cases = ([np.zeros(1, np.int32)], [np.full(1, 3, np.int32)]) if form == "batch" else ([(np.arange(n_state) % 2 * 2).astype(np.int32)],)
    for (step_host,) in step_cases:
        want_rows = _expect(d, form, R, step_host)
        logits = torch.from_numpy(x[:R]).to(dev).clone()
        state = torch.from_numpy(d["stale"]).to(dev).clone()
        step = torch.from_numpy(step_host).to(dev)
        cur = torch.full((n_state,), -7, dtype=I64, device=dev)
        req_state = torch.full((d["n_req"],), -5, dtype=I32, device=dev)
        flag = torch.zeros(1, dtype=I32, device=dev)
        a = ops.constraint_args(T, logits, step, d["finished"], cur, state, d["start"], ws, out_row=d["out_row"],
                                slot_of_row=d["slot_of_row"], request_state=req_state, flag=flag)
        ops.constraint_mask(a)
        torch.cuda.synchronize()
        got = logits.cpu().numpy()
        for r, w in enumerate(want_rows):
            want = x[r].copy()
            if w is not None:
                want[~allowed[w[2]]] = -np.inf
            assert np.array_equal(got[r].view(np.uint32), want.view(np.uint32)), (r, w)
        assert torch.equal(state.cpu(), torch.from_numpy(d["stale"])) and flag.item() == 0  # the mask writes no state
        # ---- advance on hand-made tokens: an allowed one for every live row
        toks = cur.cpu().numpy()
        want_state, want_req = d["stale"].copy(), np.full(d["n_req"], -5, np.int32)
        for i, w in enumerate(want_rows):
            if w is not None:
                ok = np.flatnonzero(allowed[w[2]])
                toks[w[0]] = ok[(i * 7919) % ok.size]
                want_state[w[0]] = want_req[w[1]] = C.next(w[2], toks[w[0]])
                assert want_state[w[0]] >= 0
        cur.copy_(torch.from_numpy(toks))
        ops.constraint_advance(a)
        torch.cuda.synchronize()
        assert flag.item() == 0
        assert np.array_equal(state.cpu().numpy(), want_state) and np.array_equal(req_state.cpu().numpy(), want_req)
        assert np.array_equal(logits.cpu().numpy().view(np.uint32), got.view(np.uint32))  # the advance writes no score
        # ---- a token its state does not allow: the flag is set, the state stays the one the mask used; the other rows advance
        bad = next((w for w in want_rows if w is not None and w[2] != FREE), None)
        if bad is None:
            continue
        state.copy_(torch.from_numpy(d["stale"]))
        logits.copy_(torch.from_numpy(x[:R]))
        ops.constraint_mask(a)
        toks[bad[0]] = np.flatnonzero(~allowed[bad[2]])[-1]
        cur.copy_(torch.from_numpy(toks))
        ops.constraint_advance(a)
        torch.cuda.synchronize()
        want_state[bad[0]] = want_req[bad[1]] = bad[2]
        assert flag.item() == 1
        assert np.array_equal(state.cpu().numpy(), want_state) and np.array_equal(req_state.cpu().numpy(), want_req)
        toks[bad[0]] = V + 5  # an id outside the vocabulary is not allowed either, and is never used as an index
        flag.zero_()
        state.copy_(torch.from_numpy(d["stale"]))
        ops.constraint_mask(a)
        cur.copy_(torch.from_numpy(toks))
        ops.constraint_advance(a)
        torch.cuda.synchronize()
        assert flag.item() == 1 and np.array_equal(state.cpu().numpy(), want_state)


def test_a_request_outside_the_start_table_is_inert(gpu):
    from tcavt_amd import ops

    dev, V, R = gpu["device"], 1000, 4
    C, allowed, x = _constraint(V)
    T = ops.ConstraintTable(C.token_class, C.trans, dev).build()
    logits = torch.from_numpy(x[:R]).to(dev).clone()
    z = torch.zeros(R, dtype=I32, device=dev)
    out_row = torch.tensor([0, 9, 1, -1], dtype=I64, device=dev)  # 4 start states: 9 and -1 name none of them
    start = torch.full((4,), ONLY_FIRST, dtype=I32, device=dev)
    state, flag = torch.full((R,), MIXED, dtype=I32, device=dev), torch.zeros(1, dtype=I32, device=dev)
    cur = torch.zeros(R, dtype=I64, device=dev)
    ws = torch.empty(ops.constraint_workspace_bytes(R), dtype=torch.uint8, device=dev)
    a = ops.constraint_args(T, logits, z, z.clone(), cur, state, start, ws, out_row=out_row, flag=flag)
    ops.constraint_mask(a)
    ops.constraint_advance(a)
    torch.cuda.synchronize()
    got = logits.cpu().numpy()
    for r in range(R):
        want = x[r].copy()
        if r in (0, 2):
            want[~allowed[ONLY_FIRST]] = -np.inf
        assert np.array_equal(got[r].view(np.uint32), want.view(np.uint32))
    assert flag.item() == 2 and state.cpu().tolist() == [2, MIXED, 2, MIXED]  # (ONLY_FIRST on token 0 leads to state 2)
