"""Grouped admissions of the slot pool on the GPU (generate_pool(admit_group=G)): tcavt_slot_admit_group as a byte copy that never
faults on a bad slot, tcavt_sample_logits_rows against tcavt_sample_logits_slots, and the model: a full group against generate_batch,
independence of a request from its group (row, partners, pad rows, schedule, slot), a refilled slot's logits against the oracle,
eager against replayed admissions, and admit_group = 1 as today's path.  Token ids and cache bytes are held bit-exact."""
import ctypes

import numpy as np
import pytest
import torch

from test_generate_pool_gpu import GUARD, _awkward_rows, _guarded, _setup, _state
from tests.util import rel_err

pytestmark = pytest.mark.gpu

IDX = [0, 1, 2, 1, 0, 2, 1]  # the fixture's three requests as a list of seven


# ------------------------------------------------------------------------------------------------
# 1. the grouped admission is a byte copy
# ------------------------------------------------------------------------------------------------
LAYERS, NKV, G_, S_, SRC_LMAX, ROWS, KV_LMAX, N_IDS, CAP, N_IMAGE = 2, 2, 3, 4, 5, 5, 9, 4, 9, 1
F16_NAMES = ("src_k", "src_v", "dst_k", "dst_v")
KV8_NAMES = ("src_k_codes", "src_k_scales", "src_v_codes", "src_v_scales", "dst_k_codes", "dst_k_scales", "dst_v_codes", "dst_v_scales")


def _admit_case(dev, form):
    gen = torch.Generator().manual_seed(11)
    if form == "kv8":
        per = (64, 2, 64, 2)
        src = [_guarded(dev, (LAYERS, G_, NKV, SRC_LMAX, p), gen=gen) for p in per]
        dst = [_guarded(dev, (LAYERS, S_, NKV, KV_LMAX, p)) for p in per]
        src_t, dst_t = [v for _, v in src], [v for _, v in dst]
    else:
        dt = torch.float16 if form == "fp16" else torch.bfloat16
        src = [_guarded(dev, (LAYERS, G_, SRC_LMAX, NKV * 64 * 2), gen=gen) for _ in range(2)]
        dst = [_guarded(dev, (LAYERS, S_, KV_LMAX, NKV * 64 * 2)) for _ in range(2)]
        src_t, dst_t = [v.view(dt) for _, v in src], [v.view(dt) for _, v in dst]
    i32, i64 = torch.int32, torch.int64
    rows = dict(prompt_ids=torch.randint(0, 512, (G_, N_IDS), generator=gen).to(dev), kv_len=torch.tensor([4, 5, 3], dtype=i32, device=dev),
                max_new_value=torch.tensor([50, 51, 52], dtype=i32, device=dev),
                out_row_value=torch.tensor([123456789012, 5, 7], dtype=i64, device=dev))
    st = dict(history=torch.full((S_, CAP), -3, dtype=i64, device=dev), hist_len=torch.full((S_,), 11, dtype=i32, device=dev),
              step=torch.full((S_,), 12, dtype=i32, device=dev), max_new=torch.full((S_,), 13, dtype=i32, device=dev),
              out_row=torch.full((S_,), 14, dtype=i64, device=dev), pos=torch.full((S_,), 15, dtype=i32, device=dev),
              finished=torch.full((S_,), 1, dtype=i32, device=dev), cur_tok=torch.full((S_,), 17, dtype=i64, device=dev))
    return src, dst, src_t, dst_t, rows, st


def _want_bytes(form, src, dst, placed):
    """placed: {row of the group: slot}.  -> the whole destination buffers (guards included) as they must read afterwards."""
    want = []
    for (db, dv), (_, sv) in zip(dst, src):
        w = dv.clone()
        for g, s in placed.items():
            if form == "kv8":
                w[:, s, :, :ROWS] = sv[:, g, :, :ROWS]
            else:
                w[:, s, :ROWS] = sv[:, g, :ROWS]
        full = db.clone()
        full[GUARD:GUARD + w.numel()] = w.reshape(-1)
        want.append(full)
    return want


def _check_admitted(dst, want, st, before, rows, placed):
    for (db, _), w in zip(dst, want):
        assert torch.equal(db, w)  # the copied rows are the source's; every other byte, guards included, is the sentinel
    for g, s in placed.items():
        assert torch.equal(st["history"][s, :N_IDS], rows["prompt_ids"][g]) and (st["history"][s, N_IDS:] == -3).all()
        got = {k: int(st[k][s]) for k in ("hist_len", "pos", "step", "finished", "max_new", "out_row")}
        kl = int(rows["kv_len"][g])
        assert got == dict(hist_len=kl - N_IMAGE, pos=kl, step=0, finished=0, max_new=int(rows["max_new_value"][g]),
                           out_row=int(rows["out_row_value"][g]))
    for k in st:
        for s in set(range(S_)) - set(placed.values()):
            assert torch.equal(st[k][s], before[k][s]), (k, s)  # the state of an untouched slot
    assert torch.equal(st["cur_tok"], before["cur_tok"])  # cur_tok everywhere


@pytest.mark.parametrize("form", ["fp16", "bf16", "kv8"])
def test_admit_group_is_a_byte_copy(gpu, form):
    from tcavt_amd import capi, ops

    dev = gpu["device"]
    i32 = torch.int32
    for slots, placed, flag_want in (([2, -1, 0], {0: 2, 2: 0}, 0), ([2, 7, 0], {0: 2, 2: 0}, 1)):
        src, dst, src_t, dst_t, rows, st = _admit_case(dev, form)
        want = _want_bytes(form, src, dst, placed)
        before = {k: v.clone() for k, v in st.items()}
        slot = torch.tensor(slots, dtype=i32, device=dev)
        flag = torch.zeros(1, dtype=i32, device=dev)
        ops.slot_admit_group(src_t, dst_t, slot, ROWS, SRC_LMAX, KV_LMAX, LAYERS, S_, NKV, rows["prompt_ids"], rows["kv_len"], N_IMAGE,
                             rows["max_new_value"], rows["out_row_value"], flag, **st)
        torch.cuda.synchronize()  # (a bad slot: the run ends clean)
        _check_admitted(dst, want, st, before, rows, placed)
        assert int(flag.item()) == flag_want
    # ---- host refusals: TCAVT_ERR_ARG and nothing launched
    src, dst, src_t, dst_t, rows, st = _admit_case(dev, form)
    flag = torch.zeros(1, dtype=i32, device=dev)
    slot = torch.tensor([2, -1, 0], dtype=i32, device=dev)
    untouched = [db.clone() for db, _ in dst]
    before = {k: v.clone() for k, v in st.items()}
    other = [_guarded(dev, (64,))[1] for _ in range(8)]

    def args(**kw):
        a = capi.SlotAdmitGroupArgs()
        if form == "kv8":
            mine = dict(zip(KV8_NAMES, src_t + dst_t))
        else:
            mine = dict(zip(F16_NAMES, src_t + dst_t))
        for k, v in {**mine, **rows, **st}.items():
            setattr(a, k, v.data_ptr())
        a.slot, a.bad_slot_flag = slot.data_ptr(), flag.data_ptr()
        a.n_layers, a.S, a.G, a.rows, a.src_lmax, a.kv_lmax, a.nkv, a.dtype16 = LAYERS, S_, G_, ROWS, SRC_LMAX, KV_LMAX, NKV, capi.F16
        a.n_ids, a.hist_cap, a.n_image = N_IDS, CAP, N_IMAGE
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    first = (KV8_NAMES if form == "kv8" else F16_NAMES)[0]
    mixed = dict(zip(F16_NAMES if form == "kv8" else KV8_NAMES, (t.data_ptr() for t in other)))
    for kw, msg in ((dict(rows=0), b"rows = 0"), (dict(rows=6), b"rows = 6"), (mixed, b"exclude each other"),
                    ({first: src_t[0].data_ptr() + 8}, b"16-byte aligned")):
        assert capi.lib().tcavt_slot_admit_group(ctypes.byref(args(**kw)), capi.stream_ptr()) == 1
        err = capi.lib().tcavt_last_error()
        assert err.startswith(b"slot_admit_group:") and msg in err, err
    torch.cuda.synchronize()
    for (db, _), w in zip(dst, untouched):
        assert torch.equal(db, w)
    for k in st:
        assert torch.equal(st[k], before[k]), k
    assert int(flag.item()) == 0


# ------------------------------------------------------------------------------------------------
# 2. the rows sampler is the slots sampler
# ------------------------------------------------------------------------------------------------
STATE_KEYS = ("history", "hist_len", "step", "max_new", "out_row", "cur", "pos", "finished", "out")


def _rows_call(ops, logits, slot_of_row, sp, st, advance_pos=True, workspace=None):
    ops.sample_logits_rows(logits, slot_of_row, st["history"], st["hist_len"], sp, st["step"], st["max_new"], st["out_row"], st["cur"],
                           st["pos"], st["finished"], st["out"], advance_pos=advance_pos, workspace=workspace)


def _same_logits(a, b):
    return torch.equal(torch.isinf(a), torch.isinf(b)) and torch.equal(torch.nan_to_num(a, neginf=0.0), torch.nan_to_num(b, neginf=0.0))


@pytest.mark.parametrize("two_stage", [False, True], ids=["one_stage", "two_stage"])
@pytest.mark.parametrize("V", [512, 50000])
def test_rows_sampler_equals_the_slots_entry(gpu, V, two_stage):
    from tcavt_amd import capi, ops

    dev = gpu["device"]
    _, cap, base, hist0, hl0 = _awkward_rows(V)
    sel = [0, 1, 2, 3, 5]  # five of the awkward rows (ties, a constant row, three finite scores, 300 equal maxima)
    base, hist0, hl0 = base[sel], hist0[sel], hl0[sel]
    S = 5
    steps, out_rows = [3, 0, 7, 2, 5], [3, 0, 7, 2, 9]
    sp = capi.SampleParams(0.9, 0.9, 1.2, 40, 3, 1, -1, 0, 1234)  # sampling on, penalty and n-gram ban in place
    i32 = torch.int32

    def fresh():
        st = _state(dev, S, cap, hist0, hl0, steps, out_rows, out_cap=12, sentinel=-9)
        st["pos"] += torch.arange(S, dtype=i32, device=dev) * 3 + 2
        return st

    def ws(n):
        return ops.sample_workspace(n, dev) if two_stage else None

    def clean(w, n):
        return w is None or int(w[:64 + 4 * n].sum().item()) == 0

    # ---- (a) the identity map over S = G = 5: tokens and every state array equal the slots entry, twice in a row
    res = []
    for rows_entry in (False, True):
        logits, st, w = base.clone().to(dev), fresh(), ws(S)
        ident = torch.arange(S, dtype=i32, device=dev)
        for _ in range(2):
            if rows_entry:
                _rows_call(ops, logits, ident, sp, st, workspace=w)
            else:
                ops.sample_logits_slots(logits, st["history"], st["hist_len"], sp, st["step"], st["max_new"], st["out_row"], st["cur"],
                                        st["pos"], st["finished"], st["out"], advance_pos=True, workspace=w)
        torch.cuda.synchronize()
        assert clean(w, S)
        res.append((logits.cpu(), {k: st[k].cpu() for k in STATE_KEYS}))
    assert _same_logits(res[0][0], res[1][0])
    for k in STATE_KEYS:
        assert torch.equal(res[0][1][k], res[1][1][k]), k
    assert res[1][1]["step"].tolist() == [s + 2 for s in steps] and int((res[1][1]["out"] != -9).sum()) == 2 * S

    # ---- (b) three rows mapped to slots [4, 0, 2]: three S = 1 calls of the existing entry on views that start at those slots
    slots = [4, 0, 2]
    lg_a, st_a, w1 = base[slots].clone().to(dev), fresh(), ws(1)
    for g, s in enumerate(slots):
        ops.sample_logits_slots(lg_a[g:g + 1], st_a["history"][s:s + 1], st_a["hist_len"][s:], sp, st_a["step"][s:], st_a["max_new"][s:],
                                st_a["out_row"][s:], st_a["cur"][s:], st_a["pos"][s:], st_a["finished"][s:], st_a["out"], advance_pos=True,
                                workspace=w1)
    lg_b, st_b, w3 = base[slots].clone().to(dev), fresh(), ws(3)
    _rows_call(ops, lg_b, torch.tensor(slots, dtype=i32, device=dev), sp, st_b, workspace=w3)
    torch.cuda.synchronize()
    assert clean(w3, 3) and _same_logits(lg_a.cpu(), lg_b.cpu())
    for k in STATE_KEYS:
        assert torch.equal(st_a[k], st_b[k]), k
    assert st_b["step"].tolist() == [4, 0, 8, 2, 6]

    # ---- (c) [4, -1, 2] (and an entry beyond S): the unmapped row and every unmapped slot are untouched; the workspace stays usable
    for hole in (-1, S):
        lg_c, st_c = base[slots].clone().to(dev), fresh()
        before = {k: st_c[k].clone() for k in STATE_KEYS}
        _rows_call(ops, lg_c, torch.tensor([4, hole, 2], dtype=i32, device=dev), sp, st_c, workspace=w3)
        torch.cuda.synchronize()
        assert clean(w3, 3)
        assert torch.equal(lg_c[1].cpu(), base[slots[1]])  # bit for bit: no processor ran on it
        for k in STATE_KEYS[:-1]:
            for s in (0, 1, 3):
                assert torch.equal(st_c[k][s], before[k][s]), (k, s)
            for s in (4, 2):
                assert torch.equal(st_c[k][s], st_b[k][s]), (k, s)
        assert torch.equal(st_c["out"][out_rows[0]], before["out"][out_rows[0]]) and int((st_c["out"] != -9).sum()) == 2
    # a following tcavt_sample_logits call on the same workspace is the one a fresh workspace gives
    outs = []
    for w in (w3, ws(3)):
        lg, st = base[slots].clone().to(dev), _state(dev, 3, cap, hist0[slots], hl0[slots], [0] * 3, out_cap=12, sentinel=-9)
        step1 = torch.full((1,), 6, dtype=i32, device=dev)
        ops.sample_logits(lg, st["history"], st["hist_len"], sp, step1, st["cur"], st["pos"], st["finished"], st["out"], advance_pos=True,
                          workspace=w)
        torch.cuda.synchronize()
        assert step1.item() == 7 and clean(w, 3)
        outs.append((st["out"].cpu(), st["cur"].cpu(), st["history"].cpu()))
    assert all(torch.equal(x, y) for x, y in zip(*outs)) and int((outs[0][0] != -9).sum()) == 3


# ------------------------------------------------------------------------------------------------
# 3. the model
# ------------------------------------------------------------------------------------------------
def _pool(M, idx=None, **kw):
    g = M["g"]
    i = torch.tensor(list(range(3)) if idx is None else idx, device=g["input_ids"].device)
    out = M["m"].mllm.generate_pool(g["vision_emb"][i], g["input_ids"][i], g["attention_mask"][i], **kw)
    torch.cuda.synchronize()
    return out.cpu()


def test_full_group_equals_generate_batch(gpu):
    """R = S = G = 3: the same B = 3 prefill, the same B = 3 step and the same Philox rows as generate_batch."""
    M = _setup(gpu["device"])
    g, N = M["g"], 10
    for kv in ("fp16", "fp8"):
        kw = dict(do_sample=True, seed=11, kv_cache=kv)
        want = M["m"].mllm.generate_batch(g["vision_emb"], None, max_new_tokens=N, input_ids=g["input_ids"],
                                          attention_mask=g["attention_mask"], **kw)
        torch.cuda.synchronize()
        got = _pool(M, max_new_tokens=N, slots=3, admit_group=3, **kw)
        M["m"].mllm.check_flags()
        assert M["m"].mllm.pool_stats["groups"] == [((0, 1, 2), (0, 1, 2), 0)]
        assert torch.equal(got, want.cpu()), kv


def _placement(groups, G):
    """request -> (row in its group, partners, pad rows beside it)"""
    return {r: (reqs.index(r), tuple(q for q in reqs if q != r), G - len(reqs)) for reqs, _, _ in groups for r in reqs}


@pytest.mark.parametrize("opts", [dict(), dict(kv_cache="fp8"), dict(decode_weights="fp8", kv_cache="fp8")],
                         ids=["fp16", "kv8", "w8_kv8"])
def test_a_request_does_not_depend_on_its_group(gpu, opts):
    """R = 7, slots 4, G = 2, sampling on, seed 5.  Run A: budgets of 12; run B: request 0's budget at 3 (one slot idles until the
    other three end: the groups of B enter other slots' company, at the same width); run C: requests 0 and 1 at 3, so that the
    group (4, 5) enters at another time, beside requests 2 and 3 mid-answer.
    With first-in-first-out groups of a fixed width a request's row and partners follow from its place in the LIST alone (row =
    r mod G), so no choice of budgets moves a request to another row: what differs between A, B and C is the schedule and the
    neighbouring slots.  The row / partner / pad-row independence is therefore shown on requests of EQUAL CONTENT inside the list
    (IDX repeats the fixture's three requests): request content 1 sits in row 1 beside content 0, in row 1 beside content 2, and in
    row 0 beside a pad row; under greedy selection (no Philox row involved) their tokens must be identical."""
    M = _setup(gpu["device"])
    mm = M["m"].mllm
    kw = dict(slots=4, admit_group=2, do_sample=True, seed=5, **opts)
    a = _pool(M, IDX, max_new_tokens=[12] * 7, **kw)
    grp_a = list(mm.pool_stats["groups"])
    b = _pool(M, IDX, max_new_tokens=[3] + [12] * 6, **kw)
    grp_b = list(mm.pool_stats["groups"])
    c = _pool(M, IDX, max_new_tokens=[3, 3] + [12] * 5, **kw)
    grp_c = list(mm.pool_stats["groups"])
    mm.check_flags()
    assert [reqs for reqs, _, _ in grp_a] == [(0, 1), (2, 3), (4, 5), (6,)]
    assert _placement(grp_a, 2) == _placement(grp_b, 2) == _placement(grp_c, 2)  # (row = r mod G: see the docstring)
    assert grp_a[3][0] == (6,) and _placement(grp_a, 2)[6] == (0, (), 1)  # the tail sits beside a pad row
    # the schedule differs: in C the group (4, 5) enters early, beside requests 2 and 3 mid-answer; in A and B after they ended
    assert grp_c[2][2] < 11 <= grp_a[2][2] and grp_c[2][2] < grp_b[2][2]
    # requests of equal content in different rows, with different partners, beside a pad row
    content = {r: IDX[r] for r in range(7)}
    pl = _placement(grp_a, 2)
    seen = {(pl[r][0], tuple(content[q] for q in pl[r][1]), pl[r][2]) for r in range(7) if content[r] == 1}
    assert seen == {(1, (0,), 0), (1, (2,), 0), (0, (), 1)}
    assert tuple(a.shape) == tuple(b.shape) == tuple(c.shape) == (7, 12)
    assert torch.equal(a[1:], b[1:])
    assert torch.equal(a[0, :3], b[0, :3]) and (b[0, 3:] == 0).all()
    assert torch.equal(a[2:], c[2:]) and torch.equal(a[:2, :3], c[:2, :3]) and (c[:2, 3:] == 0).all()
    assert ((a >= 0) & (a < M["cfg"].llama.vocab)).all()
    a2 = _pool(M, IDX, max_new_tokens=[12] * 7, **kw)
    assert torch.equal(a, a2)
    d = _pool(M, IDX, max_new_tokens=[12] * 7, **{**kw, "seed": 6})
    assert not torch.equal(a, d)
    # greedy: equal content -> equal tokens, whatever the row, the partner or the pad row
    e = _pool(M, IDX, max_new_tokens=[12] * 7, **{**kw, "do_sample": False})
    for r in range(7):
        assert torch.equal(e[r], e[IDX[r]]), (r, IDX[r])


@pytest.mark.parametrize("kv", ["fp16", "fp8"])
def test_group_cache_does_not_depend_on_row_or_partner(gpu, kv):
    """G = 3 on three slots.  Run X, list [2, 1]: request 2 in row 0 beside request 1 (slot 0); run Y, list [0, 2]: request 2 in row 1
    beside a pad row (slot 1).  The bytes of its slot's cache rows 0 .. kv_len - 1 are equal."""
    dev = gpu["device"]
    M = _setup(dev)
    mm, ll = M["m"].mllm, M["cfg"].llama
    t = M["t"]
    Lt, N, S = t["input_ids"].shape[1], 4, 3
    L, kvl = 16 + Lt, 16 + int(t["attention_mask"][2].sum())
    Lmax = L + N
    nkv = ll.n_kv_heads
    names = [("pool.kc", 0), ("pool.vc", 0)] if kv == "fp16" else [("pool.kv8.kc", 64), ("pool.kv8.ks", 2), ("pool.kv8.vc", 64), ("pool.kv8.vs", 2)]
    st = mm.llama_wrapper.storage

    def cache_rows(slot):
        out = []
        for nm, per in names:
            if kv == "fp16":
                c = mm._ws.get(nm, (ll.layers, S, Lmax, nkv * ll.head_dim), st, dev)
                out.append(c[:, slot, :kvl].clone().view(torch.uint8).cpu())
            else:
                c = mm._ws.get(nm, (ll.layers, S, nkv, Lmax, per), torch.uint8, dev)
                out.append(c[:, slot, :, :kvl].clone().cpu())
        return out

    kw = dict(max_new_tokens=N, slots=S, admit_group=3, do_sample=False, kv_cache=kv)
    x_tok = _pool(M, [2, 1], **kw)
    assert mm.pool_stats["groups"] == [((0, 1), (0, 1), 0)]
    x = cache_rows(0)
    y_tok = _pool(M, [0, 2], **kw)
    assert mm.pool_stats["groups"] == [((0, 1), (0, 1), 0)]
    y = cache_rows(1)
    mm.check_flags()
    assert any(bool(v.any()) for v in x)
    for (nm, _), xv, yv in zip(names, x, y):
        assert torch.equal(xv, yv), nm
    assert torch.equal(x_tok[0], y_tok[1])


def test_grouped_refill_logits_match_oracle(gpu):
    """test_refilled_slot_logits_match_oracle (tests/test_generate_pool_gpu.py) with G = 2: budgets [2, 9, 7] on two slots,
    poll_every = 1.  Group (0, 1) fills both slots; request 0 ends in step 1, is seen ended after step 2, and request 2 -- a second
    group, beside a pad row, into the reused slot 0 -- chooses its tokens 2 .. 7 in steps 3 .. 8 and ends last, together with
    request 1: its slot's logits row is the one its 7th token was chosen from.  Same bar, 2e-3."""
    from oracle import generation as G

    dev = gpu["device"]
    M = _setup(dev)
    cfg, weights, t = M["cfg"], M["weights"], M["t"]
    out = _pool(M, max_new_tokens=[2, 9, 7], slots=2, admit_group=2, poll_every=1, do_sample=False, repetition_penalty=1.0,
                no_repeat_ngram_size=0)
    M["m"].mllm.check_flags()
    stats = M["m"].mllm.pool_stats
    assert [g[:2] for g in stats["groups"]] == [((0, 1), (0, 1)), ((2,), (0,))] and stats["groups"][1][2] > 0
    adm = {r: (s, at) for r, s, at in stats["admitted"]}
    assert adm[2][0] == adm[0][0] and adm[2][1] > 0  # a reused slot
    ret = {r: at for r, s, at in stats["retired"]}
    assert ret[2] == stats["steps"] == max(ret.values()) and ret[0] < ret[2]  # it ends last
    assert np.array_equal(out[2, :7].numpy(), M["fx"]["greedy_tokens"][2, :7]) and (out[2, 7:] == 0).all() and (out[0, 2:] == 0).all()
    logits = M["m"].mllm._ws.get("pool.logits", (2, cfg.llama.vocab), torch.float32, dev).cpu()
    b = 2
    n_text = int(t["attention_mask"][b].sum())
    seq = G.prefix_embeds(weights, cfg, t["vision_emb"], t["input_ids"], "fp16", b, n_text)
    for tok in out[b, :6]:
        seq = torch.cat([seq, G.token_embed(weights, tok, "fp16")[None, None]], dim=1)
    with torch.no_grad():
        ref = G.next_logits(weights, cfg, seq, "fp16")
    e = rel_err(logits[adm[2][0]], ref)
    print(f"grouped refill: slot logits vs oracle: rel_err = {e:.3e}")
    assert e < 2e-3, e
    assert int(ref.argmax()) == int(out[b, 6])


def test_group_admission_eager_equals_graph(gpu):
    M = _setup(gpu["device"])
    mm = M["m"].mllm
    outs = []
    for use_graph in (False, True):
        for poll_every in (1, 5):
            outs.append(_pool(M, IDX, max_new_tokens=[5, 9, 3, 12, 7, 4, 10], slots=4, admit_group=2, do_sample=True, seed=9,
                              use_graph=use_graph, poll_every=poll_every))
            mm.check_flags()
            assert len(mm.pool_stats["groups"]) == 4  # one eager pass, then three replays with use_graph
    for o in outs[1:]:
        assert torch.equal(outs[0], o)
    assert int((outs[0] != 0).sum()) >= 7


def test_admit_group_one_is_todays_path(gpu):
    M = _setup(gpu["device"])
    g, fx = M["g"], M["fx"]
    kw = dict(max_new_tokens=[4, 6, 5], slots=2, do_sample=True, seed=3)
    a = _pool(M, **kw)
    adm = list(M["m"].mllm.pool_stats["admitted"])
    b = _pool(M, admit_group=1, **kw)
    assert torch.equal(a, b) and adm == M["m"].mllm.pool_stats["admitted"] and M["m"].mllm.pool_stats["groups"] == []
    _pool(M, IDX, max_new_tokens=6, slots=4, admit_group=2, do_sample=True, seed=3)
    N = fx["greedy_tokens"].shape[1]
    out = M["m"].mllm.generate_batch(g["vision_emb"], None, max_new_tokens=N, input_ids=g["input_ids"], attention_mask=g["attention_mask"],
                                     do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0)
    torch.cuda.synchronize()
    M["m"].mllm.check_flags()
    assert np.array_equal(out.cpu().numpy(), fx["greedy_tokens"])
