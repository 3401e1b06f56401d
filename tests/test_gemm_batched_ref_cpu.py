"""The strided float64 reference of the batched GEMM (tests/gemm_batched_ref.py), proven on the CPU before the kernels meet it:
for every named pattern batched_ref equals the obvious einsum on contiguous per-product copies made with plain indexing, the
masks mark exactly what those copies read and write, and no two products write one element of C."""
import pytest
import torch

from tests import gemm_batched_ref as R


def _copies(flat, base, rows, cols, ld):
    """[batch, rows, cols] contiguous copies of the products' operands, one slice per row, and the set of indices they read"""
    out, seen = [], set()
    for b in base.tolist():
        out.append(torch.stack([flat[b + r * ld: b + r * ld + cols] for r in range(rows)]))
        seen.update(range(b + r * ld, b + r * ld + cols) for r in range(rows))
    return torch.stack(out), seen


def _data(n, g):
    """small integers in float64: every product is exact, so that the two ways of forming it agree bit for bit"""
    return torch.randint(-8, 9, (n,), generator=g).double()


@pytest.mark.parametrize("p", R.PATTERNS, ids=lambda p: p.name)
def test_batched_ref_is_the_per_product_einsum(p):
    g = torch.Generator().manual_seed(len(p.name) + p.M)
    a_need, w_need, c_need = R.need(p)
    if p.w_in_a >= 0:
        A = _data(max(a_need, p.w_in_a + w_need) + 8, g)
        W = A[p.w_in_a:]
    else:
        A, W = _data(a_need + 8, g), _data(w_need + 8, g)
    i = torch.arange(p.batch)
    bo, bi = i // p.batch_inner, i % p.batch_inner
    oa = bo * p.sAo + bi * p.sAi
    ow = bo * p.sWo + (bi // max(p.batch_w_group, 1)) * p.sWi
    oc = bo * p.sCo + bi * p.sCi
    ac, a_seen = _copies(A, oa, p.M, p.K, p.lda)
    wc, w_seen = _copies(W, ow, p.N, p.K, p.ldw)
    want = torch.einsum("bmk,bnk->bmn", ac, wc)
    got = R.batched_ref(A, W, p)
    assert torch.equal(got, want)
    # masks: exactly the elements the copies read / the C rows the products write
    am, wm, cm = R.masks(p, A.numel(), W.numel(), c_need + 8)
    for m, seen in ((am, a_seen), (wm, w_seen)):
        ranges = torch.zeros_like(m)
        for rg in seen:
            ranges[rg.start: rg.stop] = True
        assert torch.equal(m, ranges)
    cwant = torch.zeros(c_need + 8, dtype=torch.bool)
    for b in oc.tolist():
        for r in range(p.M):
            cwant[b + r * p.ldc: b + r * p.ldc + p.N] = True
    assert torch.equal(cm, cwant) and not bool(cm[c_need:].any()) and bool(cm[c_need - 1])
    # scatter_c puts product i's rows where the call writes them
    flat = R.scatter_c(want, p, c_need + 8)
    assert torch.isnan(flat[~cm]).all()
    for k, b in enumerate(oc.tolist()):
        for r in (0, p.M - 1):
            assert torch.equal(flat[b + r * p.ldc: b + r * p.ldc + p.N], want[k, r])


@pytest.mark.parametrize("p", R.PATTERNS + [R.MAX_BATCH], ids=lambda p: p.name)
def test_c_regions_are_pairwise_disjoint(p):
    _, _, c_need = R.need(p)
    cnt = R.c_cover_count(p, c_need)
    assert int(cnt.max()) == 1, f"{p.name}: {int((cnt > 1).sum())} elements of C written by more than one product"
    assert int(cnt.sum()) == p.batch * p.M * p.N


def test_patterns_are_what_the_issue_names():
    names = {p.name for p in R.CALL_SITES}
    assert {"xattn_scores", "xattn_pv", "v_transposed", "absorbed_scores", "gqa_scores", "gqa_dq", "gqa_dk_block"} <= names
    for p in R.PATTERNS + [R.MAX_BATCH]:
        # what tcavt_gemm_bf16 asks of a batched call
        assert p.K % 64 == 0 and p.N % 16 == 0 and p.lda % 8 == 0 and p.ldw % 8 == 0 and p.ldc % 4 == 0
        assert all(s % 8 == 0 for s in p.sA + p.sW) and all(s % 4 == 0 for s in p.sC) and p.batch % p.batch_inner == 0
        assert max(p.w_in_a, 0) % 8 == 0 and p.c_off % 4 == 0
    s, dq = R.BY_NAME["gqa_scores"], R.BY_NAME["gqa_dq"]
    assert s.batch_w_group == 2 and R.BY_NAME["gqa_scores_wg_inner"].batch_w_group == s.batch_inner
    # fewer W operands addressed with a group than without: the extent ops.gemm_batched has to ask for shrinks
    assert R.need(dq)[1] < R.need(R.BY_NAME["gqa_dq_wg0"])[1]
