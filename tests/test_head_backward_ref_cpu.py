"""The float64 references and checkers of tests/head_backward_ref.py, without a GPU:
- every closed-form reference against float64 torch autograd of the forward formula (1e-12 relative): LayerNorm, masked-softmax
  attention with the dropout mask, N-Linear, out_head, poly_embed, masked mean, the MSE loss (and the 1x1 convolution, the row
  softmax);
- every checker passes on the reference rounded once to the output type and FAILS on (i) one element moved by 4x its bound,
  (ii) two neighbouring rows swapped, (iii) the last element left at the guard value (NaN);
- the integer-regime preconditions (whole units, sums of absolute values below 2^24 units) hold for every listed case."""
import pytest
import torch

import head_backward_ref as R

F64 = torch.float64


def _close(a, b, what):
    e = ((a - b).norm() / b.norm().clamp_min(1e-300)).item()
    assert e <= 1e-12, f"{what}: {e:.3e}"


def _leaf(*ts):
    return [t.clone().requires_grad_(True) for t in ts]


# ---------------------------------------------------------------------------------------------------------------------------
# closed forms against autograd

@pytest.mark.parametrize("M,D", [(5, 65), (17, 64), (4, 2048)])
def test_layernorm_bwd_formula(M, D):
    d = R.make_ln(M, D)
    x, gamma = _leaf(d["x"], d["gamma"])
    beta = torch.zeros(D, dtype=F64, requires_grad=True)
    torch.nn.functional.layer_norm(x, (D,), gamma, beta, R.LN_EPS).backward(d["gy"])
    o = R.layernorm_bwd_ref(**d)
    _close(o["gx"].ref, x.grad, "gx")
    _close(o["ggamma"].ref, d["gg0"] + gamma.grad, "ggamma")
    _close(o["gbeta"].ref, d["gb0"] + beta.grad, "gbeta")


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("case,klen", [((2, 3, 5, 2, 4), [5, 1]), ((3, 5, 3, 1, 7), [3, 0, 2]), ((2, 31, 65, 2, 8), [64, 65])])
def test_mha_bwd_formula(case, klen, p):
    B, Lq, Lk, nh, dh = case
    d = R.make_mha(case, "realistic", klen)
    scale = R.mha_scale(dh)
    keep = R.attn_keep(B, nh, Lq, Lk, p, 5) if p else None
    if p:
        assert 0 < keep.sum().item() < keep.numel()
    q, k, v = _leaf(d["q"], d["k"], d["v"])
    m = (torch.arange(Lk)[None, :] < torch.tensor(klen)[:, None])[:, None, None, :]
    s = (q.permute(0, 2, 1, 3) @ k.permute(0, 2, 3, 1)) * scale
    P = torch.softmax(s.masked_fill(~m, -1e300), -1) * m * m.any(-1, keepdim=True)
    out = ((P * keep * R.inv_keep(p)) if p else P) @ v.permute(0, 2, 1, 3)
    out.backward(d["go"].permute(0, 2, 1, 3))
    o = R.mha_bwd_ref(**d, klen=klen, scale=scale, keep=keep, ik=R.inv_keep(p))
    for name, t, L in (("gq", q, Lq), ("gk", k, Lk), ("gv", v, Lk)):
        _close(o[name].ref, t.grad.reshape(B * L, nh * dh), name)
    for b, n in enumerate(klen):        # masked keys: exactly zero, reference and bound (up to the smallest subnormal)
        for name in ("gk", "gv"):
            rows = o[name].ref.view(B, Lk, -1)[b, n:]
            assert bool((rows == 0).all()) and bool((o[name].f32.reshape(B, Lk, -1)[b, n:] == 0).all())


@pytest.mark.parametrize("case", [(2, 3, 5, 7), (5, 8, 1, 7), (20, 3, 18, 30)])
def test_nlinear_bwd_formula(case):
    d = R.make_nl(case, "realistic")
    x, W = _leaf(d["inp"], d["W"])
    bias = torch.zeros(case[1], case[3], dtype=F64, requires_grad=True)
    out = torch.einsum("cst,btc->bcs", W, x - x[:, -1:, :]) + bias[None] + x[:, -1, :][:, :, None]
    out.backward(d["g"])
    o = R.nlinear_bwd_ref(**d)
    if case[2] > 1:
        _close(o["gW"].ref, W.grad, "gW")
    else:
        assert bool((o["gW"].ref == 0).all())
    _close(o["gbias"].ref, bias.grad, "gbias")
    _close(o["gin"].ref, x.grad, "gin")   # (the last column carries the forward's direct "+ last" path: sum_s g)


def test_out_head_poly_masked_mean_mse_conv_softmax_formulas():
    d = R.make_head((3, 30, 64, 2), "realistic")
    fused, w = _leaf(d["fused"], d["w"])
    bias = torch.zeros(2, dtype=F64, requires_grad=True)
    (torch.einsum("fc,bsc->bfs", w, fused) + bias[None, :, None]).backward(d["g"])
    o = R.out_head_bwd_ref(**d)
    _close(o["gf"].ref, fused.grad, "gf"), _close(o["gw"].ref, w.grad, "gw"), _close(o["gb"].ref, bias.grad, "gb")

    d = R.make_poly((3, 5, 7), "realistic")
    w, b, pos = (torch.zeros(s, dtype=F64, requires_grad=True) for s in ((7, 2), (7,), (5, 7)))
    (torch.einsum("dk,bpk->bpd", w, d["poly"]) + b + pos[None]).backward(d["g"])
    o = R.poly_embed_bwd_ref(**d)
    _close(o["gw"].ref, w.grad, "poly gw"), _close(o["gb"].ref, b.grad, "poly gb"), _close(o["gpos"].ref, pos.grad, "gpos")

    B, P, D = 5, 17, 3
    lens = [-1, 0, 1, P, P + 3]
    gemb = R.data((B, D), "realistic", R.gen(1))
    (enc,) = _leaf(R.data((B, P, D), "realistic", R.gen(2)))
    emb = torch.stack([enc[b, :min(n, P)].mean(0) if n > 0 else enc[b, :0].sum(0) for b, n in enumerate(lens)])
    emb.backward(gemb)
    _close(R.masked_mean_bwd_ref(gemb, lens, P)["genc"].ref, enc.grad, "genc")

    d = R.make_mse(37, 30, "realistic")
    (pred,) = _leaf(d["pred"])
    r = (d["ns"][:, [1, 3]] - d["ns"][:, [0, 2]])[:, :, None]
    mn = d["ns"][:, [0, 2]][:, :, None]
    dx = (pred * r + mn) - (d["gt"] * r + mn)
    loss = (dx[:, 0] ** 2).mean() + (dx[:, 1] ** 2).mean()
    (loss * d["g_loss"] + (pred * d["g_pred"]).sum()).backward()
    _close(R.mse_grad_ref(d["pred"], d["gt"], d["ns"], d["g_loss"], d["g_pred"])["g"].ref, pred.grad, "mse both")
    _close(R.mse_grad_ref(d["pred"], d["gt"], d["ns"])["g"].ref, (pred.grad - d["g_pred"]) / d["g_loss"], "mse")

    d = R.make_conv((7, 3, 9, 2), "realistic")
    w, b = (torch.zeros(s, dtype=F64, requires_grad=True) for s in ((3, 2), (3,)))
    (torch.einsum("cf,bft->btc", w, d["x"]) + b).backward(d["gxp"])
    o = R.conv1x1_bwd_ref(**d)
    _close(o["gw"].ref, w.grad, "conv gw"), _close(o["gb"].ref, b.grad, "conv gb")

    d = R.make_sm(5, 100, "realistic")
    (s,) = _leaf(torch.randn(5, 100, dtype=F64))
    # dS = scale P (dP - sum P dP) is the softmax Jacobian at P applied to dP: check it at an exact softmax P
    P = torch.softmax(s * d["scale"], 1)
    (P * d["dP"]).sum().backward()
    _close(R.softmax_bwd_rows_ref(P.detach(), d["dP"], d["scale"], 128)["dS"].ref[:, :100], s.grad, "softmax rows")


# ---------------------------------------------------------------------------------------------------------------------------
# checker sensitivity and the integer preconditions, over every listed case

def _all_outs():
    """(what, regime, Out) of every case list of the GPU module (the shapes only where the data does not depend on more)"""
    for c in R.HEAD_CASES:
        for rg in R.REGIMES:
            yield from ((f"out_head_bwd {c} {rg} {k}", rg, o) for k, o in R.out_head_bwd_ref(**R.make_head(c, rg)).items())
    for c in R.NL_CASES:
        for rg in ["integer"] + (["realistic"] if c in R.NL_REALISTIC else []):
            yield from ((f"nlinear_bwd {c} {rg} {k}", rg, o) for k, o in R.nlinear_bwd_ref(**R.make_nl(c, rg)).items())
    for c in R.CONV_CASES:
        for rg in R.REGIMES:
            yield from ((f"conv1x1_bwd {c} {rg} {k}", rg, o) for k, o in R.conv1x1_bwd_ref(**R.make_conv(c, rg)).items())
    for c in R.POLY_CASES:
        for rg in R.REGIMES:
            yield from ((f"poly_embed_bwd {c} {rg} {k}", rg, o) for k, o in R.poly_embed_bwd_ref(**R.make_poly(c, rg)).items())
    for M, N in R.COLSUM_CASES:
        d = R.make_colsum(M, N, None)
        yield f"colsum {(M, N)}", "integer", R.colsum_ref(d["g"])["out"]
        yield f"colsum {(M, N)} accumulate", "integer", R.colsum_ref(d["g"], d["init"])["out"]
    for c in R.LN_CASES:
        yield from ((f"layernorm_bwd {c} {k}", "realistic", o) for k, o in R.layernorm_bwd_ref(**R.make_ln(*c)).items())
    for B, P, D in R.MM_CASES:
        lens = R.rotated(R.MM_LENS, B, 3, P)
        yield f"masked_mean_bwd {(B, P, D)}", "realistic", R.masked_mean_bwd_ref(R.data((B, D), "realistic", R.gen(B)), lens, P)["genc"]
    for B, To in R.MSE_CASES:
        for rg in ["realistic"] + (["integer"] if (B, To) == (4, 32) else []):
            d = R.make_mse(B, To, rg)
            yield f"mse_grad {(B, To)} {rg}", rg, R.mse_grad_ref(d["pred"], d["gt"], d["ns"], unit=d["unit"])["g"]
            yield f"mse_grad_seeded {(B, To)} {rg}", rg, R.mse_grad_ref(d["pred"], d["gt"], d["ns"], d["g_loss"], d["g_pred"], d["unit"])["g"]
    for rows in R.SM_ROWS:
        for nv, no in R.SM_COLS:
            for rg in R.REGIMES:
                d = R.make_sm(rows, nv, rg)
                yield f"softmax_bwd_rows {(rows, nv, no)} {rg}", rg, R.softmax_bwd_rows_ref(d["P"], d["dP"], d["scale"], no, d["unit"])["dS"]
    for c in R.MHA_CASES:
        kl = R.rotated(R.MHA_KLENS, c[0], 3, c[2])
        o = R.mha_bwd_ref(**R.make_mha(c, "realistic", kl), klen=kl, scale=R.mha_scale(c[4]))
        yield from ((f"mha_bwd {c} key_len={kl} {k}", "realistic", v) for k, v in o.items())
    for c in R.MHA_DROP_CASES:
        for p in R.MHA_DROP_P:
            B, Lq, Lk, nh, dh = c
            keep = R.attn_keep(B, nh, Lq, Lk, p, 9)
            assert 0 < keep.sum().item() < keep.numel(), "the mask must both keep and drop"
            o = R.mha_bwd_ref(**R.make_mha(c, "realistic"), klen=[Lk] * B, scale=R.mha_scale(dh), keep=keep, ik=R.inv_keep(p))
            yield from ((f"mha_bwd {c} p={p} {k}", "realistic", v) for k, v in o.items())
    for c in R.MHA_ONE_KEY:
        for p in (0.0, 0.5):
            B, Lq, Lk, nh, dh = c
            keep = R.attn_keep(B, nh, Lq, Lk, p, 9) if p else None
            o = R.mha_bwd_ref(**R.make_mha(c, "integer"), klen=[1] * B, scale=R.mha_scale(dh), keep=keep, ik=R.inv_keep(p))
            yield from ((f"mha_bwd one key {c} p={p} {k}", "integer", v) for k, v in o.items())
    for c, scale, kl in R.MHA_UNIFORM:
        d = R.make_mha(c, "integer")
        d["q"] = torch.zeros_like(d["q"])
        o = R.mha_bwd_ref(**d, klen=kl or [c[2]] * c[0], scale=scale, unit=scale / c[2] ** 2)
        yield from ((f"mha_bwd uniform {c} {k}", "integer", v) for k, v in o.items())


_OUTS = None


def _outs():
    global _OUTS
    if _OUTS is None:
        _OUTS = list(_all_outs())
    return _OUTS


def test_integer_preconditions_hold():
    n = 0
    for what, regime, o in _outs():
        if regime == "integer":
            assert o.exact_ok(), what
            n += 1
    assert n > 100


def test_planted_attention_values():
    """(a) one key: dQ = dK = 0, dV[0] = sum_i keep_i / (1 - p) dO[i];  (b) q = 0: dK = 0"""
    for what, regime, o in _outs():
        if "one key" in what and (what.endswith("gq") or what.endswith("gk")):
            assert bool((o.ref == 0).all()), what
        if "uniform" in what and what.endswith("gk"):
            assert bool((o.ref == 0).all()), what
        if "one key" in what and what.endswith("gv"):
            assert bool((o.ref != 0).any()), what


def test_checkers_pass_on_the_rounded_reference():
    for what, regime, o in _outs():
        R.check(o.rounded(), o, regime, what)


def _rows(t):
    return t.reshape(t.shape[0], -1) if t.dim() > 1 and t.shape[0] > 1 else t.reshape(-1, 1)


def test_checkers_fail_on_planted_errors():
    moved = swapped = guard = 0
    for what, regime, o in _outs():
        base = o.rounded().double()
        step = 4 * o.bound() if regime == "realistic" else torch.full_like(base, o.unit)
        # (i) one element moved by 4x its bound (the middle one, and the last)
        for i in {base.numel() // 2, base.numel() - 1}:
            g = base.clone().reshape(-1)
            g[i] += step.reshape(-1)[i]
            if o.dt != R.F32:           # (a 16-bit output holds the moved value only after rounding: move by 4 of its ulps too)
                g[i] = base.reshape(-1)[i] + max(step.reshape(-1)[i].item(), 4 * R._ulp(base.reshape(-1)[i:i + 1], o.dt).item())
            with pytest.raises(AssertionError):
                R.check(g.reshape(base.shape), o, regime, what + " moved")
            moved += 1
        # (ii) two neighbouring rows swapped (the first pair that differs by more than the bound somewhere)
        r, b = _rows(base), _rows(o.bound())
        for i in range(r.shape[0] - 1):
            if bool(((r[i] - r[i + 1]).abs() > 2 * torch.maximum(b[i], b[i + 1])).any()):
                g = r.clone()
                g[[i, i + 1]] = r[[i + 1, i]]
                with pytest.raises(AssertionError):
                    R.check(g.reshape(base.shape), o, regime, what + " swapped")
                swapped += 1
                break
        # (iii) the last element of a tail left at the guard value
        g = base.clone().reshape(-1)
        g[-1] = float("nan")
        with pytest.raises(AssertionError):
            R.check(g.reshape(base.shape), o, regime, what + " guard")
        guard += 1
    assert moved > 300 and swapped > 200 and guard > 300
