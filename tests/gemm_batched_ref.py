"""Float64 reference of tcavt_gemm_bf16's batched form and the stride patterns of its call sites -- TEST INFRASTRUCTURE ONLY.

The address rule is the one of include/tcavt.h (tcavt_gemm_args.batch .. batch_w_group): product i of `batch` has
bo = i // batch_inner, bi = i % batch_inner and uses

    A + bo * sAo + bi * sAi                                   [M][lda], K columns
    W + bo * sWo + (bi // max(batch_w_group, 1)) * sWi        [N][ldw], K columns
    C + bo * sCo + bi * sCi                                   [M][ldc], N columns

all in elements from the pointers the call passes.  `args` below is anything with the fields of capi.GemmArgs that the rule
names (a Pattern, or a GemmArgs itself); the flat buffers start AT those pointers.  batched_ref forms every product with
torch.as_strided on float64 copies of the flat buffers; masks() marks the elements some product addresses; scatter_c lays
per-product results out as the call's C.  tests/test_gemm_batched_ref_cpu.py proves the three against plain indexing.
"""
import dataclasses

import torch


@dataclasses.dataclass(frozen=True)
class Pattern:
    """One batched call: the GemmArgs fields of the address rule, where W and C point, and the epilogue of the call site."""
    name: str
    M: int
    N: int
    K: int
    batch: int
    batch_inner: int
    batch_w_group: int
    lda: int
    ldw: int
    ldc: int
    sA: tuple
    sW: tuple
    sC: tuple
    w_in_a: int = -1     # >= 0: W is this many elements into A's buffer (the k column block of one q|k|v buffer)
    c_off: int = 0       # C points this many elements into its buffer (a column block of a wider matrix)
    c_total: int = 0     # elements of the whole matrix C points into (0: what the products need)
    acc_scale: float = 1.0
    bias_row: bool = False
    site: str = ""

    sAo = property(lambda s: s.sA[0])
    sAi = property(lambda s: s.sA[1])
    sWo = property(lambda s: s.sW[0])
    sWi = property(lambda s: s.sW[1])
    sCo = property(lambda s: s.sC[0])
    sCi = property(lambda s: s.sC[1])

    def fields(self):
        """the GemmArgs fields of the batched form"""
        return dict(M=self.M, N=self.N, K=self.K, lda=self.lda, ldw=self.ldw, ldc=self.ldc, batch=self.batch,
                    batch_inner=self.batch_inner, batch_w_group=self.batch_w_group, sAo=self.sAo, sAi=self.sAi, sWo=self.sWo,
                    sWi=self.sWi, sCo=self.sCo, sCi=self.sCi)

    def but(self, name, **kw):
        return dataclasses.replace(self, name=name, **kw)


def offsets(args, device=None):
    """element offsets [batch] of every product's A, W and C from the call's pointers"""
    i = torch.arange(int(args.batch), dtype=torch.int64, device=device)
    bo = torch.div(i, int(args.batch_inner), rounding_mode="floor")
    bi = i - bo * int(args.batch_inner)
    bw = torch.div(bi, max(int(args.batch_w_group), 1), rounding_mode="floor")
    return bo * int(args.sAo) + bi * int(args.sAi), bo * int(args.sWo) + bw * int(args.sWi), bo * int(args.sCo) + bi * int(args.sCi)


def need(args):
    """elements the products address past the A, W and C pointers (last address + 1)"""
    oa, ow, oc = offsets(args)
    return (int(oa.max()) + (args.M - 1) * args.lda + args.K, int(ow.max()) + (args.N - 1) * args.ldw + args.K,
            int(oc.max()) + (args.M - 1) * args.ldc + args.N)


def _indices(base, rows, cols, ld):
    r = torch.arange(rows, dtype=torch.int64, device=base.device)
    c = torch.arange(cols, dtype=torch.int64, device=base.device)
    return base[:, None, None] + r[None, :, None] * ld + c[None, None, :]  # [batch, rows, cols]


def masks(args, a_len, w_len, c_len, device=None):
    """boolean masks over the flat A, W and C buffers: addressed by some product"""
    oa, ow, oc = offsets(args, device)
    out = []
    for base, rows, cols, ld, n in ((oa, args.M, args.K, args.lda, a_len), (ow, args.N, args.K, args.ldw, w_len),
                                    (oc, args.M, args.N, args.ldc, c_len)):
        m = torch.zeros(n, dtype=torch.bool, device=device)
        if n:  # (a length of 0: the caller does not want this mask)
            m[_indices(torch.unique(base), rows, cols, ld).reshape(-1)] = True
        out.append(m)
    return out


def c_cover_count(args, c_len, device=None):
    """how many products address each element of the flat C (a well-defined call has no element above 1)"""
    _, _, oc = offsets(args, device)
    idx = _indices(oc, args.M, args.N, args.ldc).reshape(-1)
    return torch.zeros(c_len, dtype=torch.int64, device=device).index_add_(0, idx, torch.ones_like(idx))


def batched_ref(A_flat, W_flat, args):
    """[batch, M, N] float64: A_i . W_i^T for every product of the call, operands read through torch.as_strided"""
    assert A_flat.dtype == torch.float64 and W_flat.dtype == torch.float64 and A_flat.dim() == 1 and W_flat.dim() == 1
    assert A_flat.stride(0) == 1 and W_flat.stride(0) == 1
    oa, ow, _ = offsets(args)
    out = torch.empty(args.batch, args.M, args.N, dtype=torch.float64, device=A_flat.device)
    for i in range(args.batch):
        # (as_strided counts its offset from the start of the storage, not of the view: a flat buffer may be a slice)
        a = torch.as_strided(A_flat, (args.M, args.K), (args.lda, 1), A_flat.storage_offset() + int(oa[i]))
        w = torch.as_strided(W_flat, (args.N, args.K), (args.ldw, 1), W_flat.storage_offset() + int(ow[i]))
        out[i] = a @ w.T
    return out


def scatter_c(vals, args, c_len, fill=float("nan")):
    """flat C image [c_len] of per-product values [batch, M, N]; elements no product addresses hold `fill`"""
    _, _, oc = offsets(args)
    flat = torch.full((c_len,), fill, dtype=vals.dtype, device=vals.device)
    for i in range(args.batch):
        torch.as_strided(flat, (args.M, args.N), (args.ldc, 1), int(oc[i])).copy_(vals[i])
    return flat


# ---------------------------------------------------------------------------------------------------------------------------
# the call sites' patterns at the smallest shapes that keep their structure: M ragged below a tile, N a multiple of 16 but not
# of every tile, more than one outer and more than one inner index

def _xattn(B=3, nh=2, To=30, L=96, Lp=128, dh=128):
    H = nh * dh
    return [
        Pattern("xattn_scores", To, Lp, dh, B * nh, nh, 1, H, H, Lp, (To * H, dh), (L * H, dh), (nh * To * Lp, To * Lp), acc_scale=0.25,
                site="ltsf.py head cross-attention: scores = q_bh . k_bh^T, heads as column slices of q and k (lda = H > K); columns "
                     "L .. Lp read the next sample's rows / the tail padding"),
        Pattern("xattn_pv", To, dh, Lp, B * nh, nh, 1, Lp, B * Lp, H, (nh * To * Lp, To * Lp), (Lp, dh * B * Lp), (To * H, dh),
                site="ltsf.py: out = p_bh . (v^T_bh)^T, W's inner stride above its outer one, C heads as column blocks of [B To, H]"),
        Pattern("absorbed_scores", To, Lp, H, B * nh, nh, 1, H, H, Lp, (To * H, B * To * H), (L * H, 0), (nh * To * Lp, To * Lp),
                acc_scale=0.25, site="ltsf.py absorbed form: q' [nh, B To, H] (inner stride above the outer one), W shared by the heads (sWi = 0)"),
    ]


def _v_transposed(B=3, L=40, Lp=64, H=128):
    return Pattern("v_transposed", H, Lp, H, B, 1, 1, H, H, B * Lp, (0, 0), (L * H, 0), (Lp, 0), bias_row=True,
                   site="ltsf.py: V^T = W_v . x_b^T + b_v[:, None], one A for all products (sA = 0), interleaved column blocks of one C")


def _gqa(B=2, nq=4, nkv=2, T=40, Tp=64, hd=64):
    nqkv, ld3 = (nq + 2 * nkv) * hd, 3 * nq * hd
    grp = nq // nkv
    scores = Pattern("gqa_scores", T, Tp, hd, B * nq, nq, grp, nqkv, nqkv, Tp, (T * nqkv, hd), (T * nqkv, hd), (nq * T * Tp, T * Tp),
                     w_in_a=nq * hd, acc_scale=0.125,
                     site="llm_backward.py 'gemm': S = q_h . k_g^T, W = the k column block of the same q|k|v buffer, w_group = nq / nkv")
    dq = Pattern("gqa_dq", T, hd, Tp, B * nq, nq, grp, Tp, B * Tp, ld3, (nq * T * Tp, T * Tp), (Tp, hd * B * Tp), (T * ld3, hd),
                 c_total=B * T * ld3, site="llm_backward.py 'gemm': dQ_h = dS_h . k_g, C = column block 0 of G3 [B T, 3 nq hd]")
    dk = Pattern("gqa_dk_block", T, hd, Tp, B * nq, nq, 1, Tp, B * Tp, ld3, (nq * Tp * Tp, Tp * Tp), (Tp, hd * B * Tp), (T * ld3, hd),
                 c_off=nq * hd, c_total=B * T * ld3, site="llm_backward.py: dK_h = dS_h^T q_h per query head, C = G3[:, nq hd:]")
    return [scores, dq, dk,
            scores.but("gqa_scores_wg_inner", batch_w_group=nq), scores.but("gqa_scores_wg0", batch_w_group=0),
            dq.but("gqa_dq_wg_inner", batch_w_group=nq), dq.but("gqa_dq_wg0", batch_w_group=0)]


def _contiguous(name, M, N, K, batch, inner, site):
    return Pattern(name, M, N, K, batch, inner, 1, K, K, N, (inner * M * K, M * K), (inner * N * K, N * K), (inner * M * N, M * N), site=site)


CALL_SITES = _xattn() + [_v_transposed()] + _gqa()
FORMS = [
    _contiguous("pipe1_batch96", 256, 256, 64, 96, 8, "4 x 96 = 384 workgroups of 128x128: launch_small counts the batch, PIPE 1"),
    _contiguous("skinny_shaped", 17, 48, 256, 6, 2, "M <= 32 and K % 256 == 0 with batch > 1: not the skinny form"),
]
MAX_BATCH = Pattern("max_batch", 16, 16, 64, 65535, 1, 1, 64, 64, 16, (0, 0), (0, 0), (256, 0),
                    site="blockIdx.y at its limit: one operand pair, 65535 contiguous C blocks")
PATTERNS = CALL_SITES + FORMS
BY_NAME = {p.name: p for p in PATTERNS + [MAX_BATCH]}
