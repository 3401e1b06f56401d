"""Tensor-level wrappers over the C ABI (one Python function per entry point).

torch is used here for device memory and the current stream only; every
computation happens inside libtcavt_hip.so.  All tensors must be CUDA(HIP)
tensors, contiguous in the layout the header documents.
"""
import ctypes

import torch

from . import capi
from .capi import BF16, EPI_BIAS, EPI_RELU, EPI_RESIDUAL, EPI_ROPE, EPI_SILU_MUL, F32, check, lib, ptr, stream_ptr

__all__ = [
    "gemm_bf16", "rmsnorm", "layernorm", "cast_bf16", "embed_fuse", "mask_to_kvlen", "attn_causal_gqa", "mha", "gemm_f32",
    "poly_embed", "masked_mean", "ltsf_front", "ltsf_decode", "transpose_ct", "out_head", "traj_metrics",
]


_ALLOW_CPU = False  # tests only: host-logic dry run with a stubbed library (tests/test_host_dryrun.py)


def _req(t, dtype, name):
    if t is None:
        return
    if not t.is_cuda and not _ALLOW_CPU:
        raise capi.TcavtError(f"{name}: tensor must live on the GPU (no CPU fallback)")
    if t.dtype != dtype:
        raise capi.TcavtError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise capi.TcavtError(f"{name}: tensor must be contiguous")


_H16 = (torch.float16, torch.bfloat16)


def _req16(t, name, like=None, rows_ok=False):
    """16-bit storage tensor (fp16 = the forward path's default, or bf16); `like`: must share that tensor's dtype.
    rows_ok: a 2-D view with unit column stride (a column slice of a wider matrix) is accepted as well."""
    if t is None:
        return
    if not t.is_cuda and not _ALLOW_CPU:
        raise capi.TcavtError(f"{name}: tensor must live on the GPU (no CPU fallback)")
    if t.dtype not in _H16 or (like is not None and t.dtype != like.dtype):
        raise capi.TcavtError(f"{name}: expected {'fp16 or bf16' if like is None else like.dtype}, got {t.dtype}")
    if not t.is_contiguous() and not (rows_ok and t.dim() == 2 and t.stride(1) == 1):
        raise capi.TcavtError(f"{name}: tensor must be contiguous")


def _need(t, numel, name):
    """Host-side guard: the buffer must hold at least what the kernel's grid will touch."""
    if t is not None and t.numel() < numel:
        raise capi.TcavtError(f"{name}: buffer has {t.numel()} elements, kernel needs {numel}")


_drop = capi.drop_spec  # dropout spec (p, seed, site) or None -> (p, seed, site) ctypes-ready


def gemm_bf16(a, w, out=None, *, out_dtype=None, bias=None, relu=False, residual=None, a2=None,
              w2=None, silu_mul=False, rope=None, tile=0, acc_scale=1.0, dropout=None, silu_preact=None, splitk_ws=None):
    """C = a @ w.T (+ a2 @ w2.T) with fused epilogue.  a [M,K], w [N,K]: both fp16 or both bf16 (the name is
    historical); out: fp32 or either 16-bit type (default: the operands' type).

    silu_preact (with silu_mul): bf16 [M, N] buffer that receives the gate|up pre-activations (for silu_mul_bwd).

    rope = (cos [L,32] f32, sin [L,32] f32, rope_cols) applies RoPE with position m % L.

    splitk_ws (M <= 32 only): uint8 device workspace (>= 64 KiB, first 16 KiB zeroed once) that lets the skinny form split K
    across workgroups -- tcavt_gemm_args.splitk_ws.
    """
    _req16(a, "gemm_bf16.a", rows_ok=True)  # (A may be a column slice: lda = its row stride)
    _req16(w, "gemm_bf16.w", like=a, rows_ok=True)
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K
    n_out = N // 2 if silu_mul else N
    if out is None:
        out = torch.empty((M, n_out), dtype=out_dtype or a.dtype, device=a.device)
    if (not out.is_cuda and not _ALLOW_CPU) or out.dim() != 2 or out.stride(1) != 1:  # a column slice of a wider buffer is fine
        raise capi.TcavtError("gemm_bf16.out: 2-D GPU tensor with unit column stride required")
    args = capi.GemmArgs()
    args.A, args.lda = a.data_ptr(), a.stride(0)
    args.W, args.ldw = w.data_ptr(), w.stride(0)
    if a2 is not None:
        _req16(a2, "gemm_bf16.a2", like=a)
        _req16(w2, "gemm_bf16.w2", like=a)
        args.A2, args.lda2 = a2.data_ptr(), a2.stride(0)
        args.W2, args.ldw2 = w2.data_ptr(), w2.stride(0)
        args.K2 = a2.shape[1]
    args.C, args.ldc = out.data_ptr(), out.stride(0)
    epi = 0
    if bias is not None:
        _req(bias, torch.float32, "gemm_bf16.bias")
        args.bias = bias.data_ptr()
        epi |= EPI_BIAS
    if relu:
        epi |= EPI_RELU
    if residual is not None:
        _req(residual, torch.float32, "gemm_bf16.residual")
        args.residual, args.ldr = residual.data_ptr(), residual.stride(0)
        epi |= EPI_RESIDUAL
    if silu_mul:
        epi |= EPI_SILU_MUL
        if silu_preact is not None:
            _req16(silu_preact, "gemm_bf16.silu_preact", like=a)
            if silu_preact.shape[0] < M or silu_preact.shape[1] < N:
                raise capi.TcavtError("gemm_bf16.silu_preact: smaller than (M, N)")
            args.silu_preact, args.ld_preact = silu_preact.data_ptr(), silu_preact.stride(0)
    if rope is not None:
        cos, sin, cols = rope
        _req(cos, torch.float32, "gemm_bf16.rope_cos")
        _req(sin, torch.float32, "gemm_bf16.rope_sin")
        args.rope_cos, args.rope_sin = cos.data_ptr(), sin.data_ptr()
        args.rope_L, args.rope_cols = cos.shape[0], cols
        epi |= EPI_ROPE
    if out.shape[0] < M or out.shape[1] < n_out:
        raise capi.TcavtError(f"gemm_bf16.out: shape {tuple(out.shape)} smaller than ({M}, {n_out})")
    if a2 is not None and (a2.shape[0] < M or w2.shape[0] < N or w2.shape[1] != a2.shape[1]):
        raise capi.TcavtError("gemm_bf16: a2/w2 shapes do not match (M, K2) / (N, K2)")
    if bias is not None:
        _need(bias, N, "gemm_bf16.bias")
    if residual is not None and (residual.shape[0] < M or residual.shape[1] < N):
        raise capi.TcavtError("gemm_bf16.residual: smaller than (M, N)")
    args.M, args.N, args.K = M, N, K
    args.out_dtype = _DT[out.dtype]
    args.in_dtype = _DT[a.dtype]
    args.epilogue = epi
    args.tile = tile
    args.acc_scale = acc_scale
    args.dropout_p, args.dropout_seed, args.dropout_site = _drop(dropout)
    if splitk_ws is not None:
        _req(splitk_ws, torch.uint8, "gemm_bf16.splitk_ws")
        args.splitk_ws, args.splitk_ws_bytes = splitk_ws.data_ptr(), splitk_ws.numel()
    check(lib().tcavt_gemm_bf16(ctypes.byref(args), stream_ptr()), "tcavt_gemm_bf16")
    return out


def silu_bwd_fusable(M, I, H):
    """Shapes for which gemm_silu_bwd exists (whole 256 x 256 tiles of the 4-wave kernel)."""
    return M % 256 == 0 and I % 256 == 0 and H % 64 == 0 and H >= 128


def gemm_silu_bwd(g, w_t, gu, out=None):
    """d(gate|up) = silu_mul_bwd(gu, g @ w_t.T) with the activation gradient never leaving the GEMM (TCAVT_EPI_SILU_BWD):
    g 16-bit [M, H] = dL/d(down_proj output), w_t [I, H] = down_proj.weight^T, gu [M, 2I] the forward's gate|up
    pre-activations (interleaved layout); out [M, 2I] (default: gu itself, in place)."""
    _req16(g, "gemm_silu_bwd.g", rows_ok=True)
    _req16(w_t, "gemm_silu_bwd.w_t", like=g, rows_ok=True)
    _req16(gu, "gemm_silu_bwd.gu", like=g, rows_ok=True)
    M, H = g.shape
    I = w_t.shape[0]
    out = gu if out is None else out
    _req16(out, "gemm_silu_bwd.out", like=g, rows_ok=True)
    if w_t.shape[1] != H or gu.shape[0] < M or gu.shape[1] < 2 * I or out.shape[0] < M or out.shape[1] < 2 * I or not silu_bwd_fusable(M, I, H):
        raise capi.TcavtError("gemm_silu_bwd: shapes (g [M,H], w_t [I,H], gu / out [M,2I]; M, I multiples of 256)")
    args = capi.GemmArgs()
    args.A, args.lda, args.W, args.ldw = g.data_ptr(), g.stride(0), w_t.data_ptr(), w_t.stride(0)
    args.C, args.ldc = out.data_ptr(), out.stride(0)
    args.silu_preact, args.ld_preact = gu.data_ptr(), gu.stride(0)
    args.M, args.N, args.K = M, I, H
    args.out_dtype = args.in_dtype = _DT[g.dtype]
    args.epilogue = capi.EPI_SILU_BWD
    check(lib().tcavt_gemm_bf16(ctypes.byref(args), stream_ptr()), "tcavt_gemm_bf16(SILU_BWD)")
    return out


def _avail(t):
    """Elements addressable from t.data_ptr() to the end of its storage."""
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: capi.F16}


def gemm_batched(a, w, out, *, M, N, K, lda, ldw, ldc, batch, inner, sA, sW, sC, bias_row=None, acc_scale=1.0,
                 tile=128, w_group=1):
    """`batch` independent products C_i = A_i . W_i^T with two-level strides (outer, inner) in elements:
    product i uses a + (i // inner) * sA[0] + (i % inner) * sA[1], likewise w and out.  a/w share a
    16-bit dtype (bf16 or fp16); out may be fp32, bf16 or fp16.  See tcavt_gemm_args (include/tcavt.h)."""
    if a.dtype != w.dtype or a.dtype not in (torch.bfloat16, torch.float16):
        raise capi.TcavtError("gemm_batched: a and w must both be bf16 or both fp16")
    outer = batch // inner
    if batch < 1 or batch % inner:
        raise capi.TcavtError("gemm_batched: batch must be a positive multiple of inner")
    for t, s, rows, ld, cols, nm in ((a, sA, M, lda, K, "a"), (w, sW, N, ldw, K, "w"), (out, sC, M, ldc, N, "out")):
        if not t.is_cuda and not _ALLOW_CPU:
            raise capi.TcavtError(f"gemm_batched.{nm}: tensor must live on the GPU")
        last_inner = (inner - 1) // max(w_group, 1) if nm == "w" else inner - 1  # w_group products share one W (0: off, as 1)
        need = (outer - 1) * s[0] + last_inner * s[1] + (rows - 1) * ld + cols
        if _avail(t) < need:
            raise capi.TcavtError(f"gemm_batched.{nm}: buffer has {_avail(t)} elements past its pointer, needs {need}")
    args = capi.GemmArgs()
    args.A, args.lda = a.data_ptr(), lda
    args.W, args.ldw = w.data_ptr(), ldw
    args.C, args.ldc = out.data_ptr(), ldc
    args.M, args.N, args.K = M, N, K
    args.out_dtype = _DT[out.dtype]
    args.in_dtype = _DT[a.dtype]
    args.acc_scale = acc_scale
    args.tile = tile
    if bias_row is not None:
        _req(bias_row, torch.float32, "gemm_batched.bias_row")
        _need(bias_row, M, "gemm_batched.bias_row")
        args.bias = bias_row.data_ptr()
        args.epilogue = capi.EPI_BIAS_ROW
    args.batch, args.batch_inner = batch, inner
    args.batch_w_group = w_group
    args.sAo, args.sAi = sA
    args.sWo, args.sWi = sW
    args.sCo, args.sCi = sC
    check(lib().tcavt_gemm_bf16(ctypes.byref(args), stream_ptr()), "tcavt_gemm_bf16(batched)")
    return out


def softmax_rows(s, p, rows, n_valid, n_out, lds, ldp, dropout=None):
    _req(s, torch.float32, "softmax_rows.s")
    if p.dtype not in (torch.bfloat16, torch.float16):
        raise capi.TcavtError("softmax_rows.p: must be bf16 or fp16")
    if _avail(s) < (rows - 1) * lds + n_valid or _avail(p) < (rows - 1) * ldp + n_out:
        raise capi.TcavtError("softmax_rows: buffer too small")
    dp, dseed, dsite = _drop(dropout)
    check(lib().tcavt_softmax_rows(ptr(s), lds, ptr(p), ldp, _DT[p.dtype], rows, n_valid, n_out, dp, dseed, dsite,
                                   stream_ptr()), "tcavt_softmax_rows")


def set_dropout_epoch(epoch):
    """Register (or, with None, clear) the device-resident int64 that every dropout kernel adds to its seed when it runs
    (fresh masks under hipGraph replay, tcavt_set_dropout_epoch).  The tensor must outlive its registration."""
    if epoch is not None:
        _req(epoch, torch.int64, "set_dropout_epoch.epoch")
        _need(epoch, 1, "set_dropout_epoch.epoch")
    check(lib().tcavt_set_dropout_epoch(ptr(epoch)), "tcavt_set_dropout_epoch")


def dropout_epoch_advance(epoch):
    _req(epoch, torch.int64, "dropout_epoch_advance.epoch")
    check(lib().tcavt_dropout_epoch_advance(ptr(epoch), stream_ptr()), "tcavt_dropout_epoch_advance")


def dropout_(x, spec):
    """In-place dropout with a (p, seed, site) spec, no-op for None: how the backward re-applies a forward mask to a
    gradient of the same shape."""
    if spec is not None:
        dropout(x, x, *spec)
    return x


def dropout(x, out, p, seed, site, add=None):
    """out = x * keep / (1 - p) (+ add) with the Philox mask of (seed, site); x/out/add share fp32, bf16 or fp16; in
    place allowed."""
    if x.dtype != out.dtype or x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise capi.TcavtError("dropout: x and out must share one of fp32 / bf16 / fp16")
    _need(out, x.numel(), "dropout.out")
    if add is not None and (add.dtype != x.dtype or add.numel() < x.numel()):
        raise capi.TcavtError("dropout.add: same dtype and at least as many elements as x")
    check(lib().tcavt_dropout(ptr(x), ptr(out), x.numel(), _DT[x.dtype], float(p), int(seed) & 0xFFFFFFFFFFFFFFFF,
                              int(site) & 0xFFFFFFFF, ptr(add), stream_ptr()), "tcavt_dropout")
    return out


def rmsnorm(x, gamma, eps, out_bf16=None, out_f32=None, out_drop=None, dropout=None):
    """out_drop (bf16, with dropout=(p, seed, site)): dropout(out_bf16) from the same pass (LoRA branch input)."""
    _req(x, torch.float32, "rmsnorm.x")
    _req(gamma, torch.float32, "rmsnorm.gamma")
    M, H = x.shape
    _need(gamma, H, "rmsnorm.gamma")
    _need(out_bf16, M * H, "rmsnorm.out_bf16")
    _need(out_f32, M * H, "rmsnorm.out_f32")
    if (out_drop is None) != (dropout is None):
        raise capi.TcavtError("rmsnorm: out_drop and dropout go together")
    _req16(out_bf16, "rmsnorm.out_bf16")
    if out_drop is not None:
        _req16(out_drop, "rmsnorm.out_drop", like=out_bf16)
        _need(out_drop, M * H, "rmsnorm.out_drop")
    dt16 = _DT[out_bf16.dtype] if out_bf16 is not None else (_DT[out_drop.dtype] if out_drop is not None else BF16)
    check(lib().tcavt_rmsnorm(ptr(x), ptr(gamma), eps, ptr(out_bf16), ptr(out_f32), M, H, ptr(out_drop),
                              *_drop(dropout), dt16, stream_ptr()), "tcavt_rmsnorm")


def layernorm(x, gamma, beta, eps=1e-5, residual=None, out_f32=None, out_bf16=None):
    _req(x, torch.float32, "layernorm.x")
    _req(residual, torch.float32, "layernorm.residual")
    M, D = x.shape
    for t, n, nm in ((gamma, D, "gamma"), (beta, D, "beta"), (residual, M * D, "residual"), (out_f32, M * D, "out_f32"),
                     (out_bf16, M * D, "out_bf16")):
        _need(t, n, "layernorm." + nm)
    _req16(out_bf16, "layernorm.out_bf16")
    check(lib().tcavt_layernorm(ptr(x), ptr(residual), ptr(gamma), ptr(beta), eps, ptr(out_f32), ptr(out_bf16), M,
                                D, _DT[out_bf16.dtype] if out_bf16 is not None else BF16, stream_ptr()), "tcavt_layernorm")


def cast16(x, out=None, dtype=torch.float16):
    """fp32 -> fp16 / bf16 copy (round to nearest even); the type is `out`'s when given."""
    _req(x, torch.float32, "cast.x")
    if out is None:
        out = torch.empty(x.shape, dtype=dtype, device=x.device)
    _req16(out, "cast.out")
    _need(out, x.numel(), "cast.out")
    check(lib().tcavt_cast_f32_16(ptr(x), ptr(out), x.numel(), _DT[out.dtype], stream_ptr()), "tcavt_cast_f32_16")
    return out


def cast_bf16(x, out=None):
    """fp32 -> bf16 (gradient-side tensors); out may also be an fp16 buffer, whose type then wins."""
    return cast16(x, out, torch.bfloat16)


def pack_weight16(w, out=None):
    """Fragment-major copy of a 16-bit weight matrix [N, K] for the skinny (decode-step) form of gemm_bf16
    (tcavt_pack_weight16; tcavt_gemm_args.w_layout = W_FRAG16): same N * K elements, every 16-row x 32-column fragment a run
    of 1 KiB in the consuming wave's lane order."""
    assert w.dim() == 2 and w.dtype in (torch.float16, torch.bfloat16) and w.stride(1) == 1
    N, K = w.shape
    if out is None:
        out = torch.empty(N * K, dtype=w.dtype, device=w.device)
    assert out.numel() == N * K and out.dtype == w.dtype and out.is_contiguous()
    capi.check(capi.lib().tcavt_pack_weight16(w.data_ptr(), w.stride(0), out.data_ptr(), N, K, capi.stream_ptr()), "pack_weight16")
    return out


def pack_weight8(w, out=None):
    """FP8 copy of a 16-bit weight matrix [N, K] for the skinny (decode-step) form of gemm_bf16 (tcavt_pack_weight8;
    tcavt_gemm_args.w_layout = W_FRAG8): uint8 [N * K + 4 * N] -- the e4m3 codes in pack_weight16's order at one byte per
    element, then the N power-of-two row scales as fp32.  quant.py is the definition."""
    assert w.dim() == 2 and w.dtype in (torch.float16, torch.bfloat16) and w.stride(1) == 1
    N, K = w.shape
    nbytes = int(capi.lib().tcavt_pack_weight8_bytes(N, K))
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    assert out.numel() == nbytes and out.dtype == torch.uint8 and out.is_contiguous()
    capi.check(capi.lib().tcavt_pack_weight8(w.data_ptr(), w.stride(0), _DT[w.dtype], out.data_ptr(), N, K, capi.stream_ptr()), "pack_weight8")
    return out


def quant_mx8(x, codes=None, scales=None):
    """MX8 image of a 16-bit matrix x [M, K] (K % 128 == 0; a column slice with unit column stride is fine): e4m3 codes uint8
    [M, K] and E8M0 scale bytes uint8 [M, K / 32], byte for byte quant.quantize_mx (tcavt_quant_mx8)."""
    _req16(x, "quant_mx8.x", rows_ok=True)
    M, K = x.shape
    if codes is None:
        codes = torch.empty((M, K), dtype=torch.uint8, device=x.device)
    if scales is None:
        scales = torch.empty((M, K // 32), dtype=torch.uint8, device=x.device)
    for t, nm, cols in ((codes, "codes", K), (scales, "scales", K // 32)):
        if t.dtype != torch.uint8 or t.dim() != 2 or t.stride(1) != 1 or t.shape[0] < M or t.shape[1] < cols or (not t.is_cuda and not _ALLOW_CPU):
            raise capi.TcavtError(f"quant_mx8.{nm}: uint8 GPU tensor of at least ({M}, {cols}) with unit column stride required")
    check(lib().tcavt_quant_mx8(ptr(x), x.stride(0), _DT[x.dtype], ptr(codes), codes.stride(0), ptr(scales), scales.stride(0), M, K,
                                stream_ptr()), "tcavt_quant_mx8")
    return codes, scales


def gemm_mx8(a8, a_scale, w8, w_scale, out, dtype16, *, epilogue=0, **fields):
    """C = dequantize_mx(a8, a_scale) @ dequantize_mx(w8, w_scale).T on the block-scaled MFMA (tcavt_gemm_mx8).  a8 [M, K], w8 [N, K]
    uint8 codes, a_scale / w_scale uint8 [.., K / 32]; out: fp32 or `dtype16` [M, N] ([M, N / 2] with SILU_MUL), or None with
    NORM_OUT for the in-place 16-bit stream.  `fields`: further tcavt_gemm_mx8_args members (tensors are passed by pointer)."""
    for t, nm in ((a8, "a8"), (a_scale, "a_scale"), (w8, "w8"), (w_scale, "w_scale")):
        if t.dtype != torch.uint8 or t.dim() != 2 or t.stride(1) != 1 or (not t.is_cuda and not _ALLOW_CPU):
            raise capi.TcavtError(f"gemm_mx8.{nm}: 2-D uint8 GPU tensor with unit column stride required")
    M, K = a8.shape
    N = w8.shape[0]
    if w8.shape[1] != K or a_scale.shape[0] < M or w_scale.shape[0] < N or a_scale.shape[1] < K // 32 or w_scale.shape[1] < K // 32:
        raise capi.TcavtError("gemm_mx8: operand / scale shapes do not match (M, K), (N, K), (.., K / 32)")
    args = capi.GemmMx8Args()
    args.A8, args.lda, args.A_scale, args.ldsa = a8.data_ptr(), a8.stride(0), a_scale.data_ptr(), a_scale.stride(0)
    args.W8, args.ldw, args.W_scale, args.ldsw = w8.data_ptr(), w8.stride(0), w_scale.data_ptr(), w_scale.stride(0)
    args.M, args.N, args.K = M, N, K
    args.dtype16, args.epilogue = _DT[dtype16], epilogue
    if out is not None:
        n_out = N // 2 if epilogue & EPI_SILU_MUL else N
        if (not out.is_cuda and not _ALLOW_CPU) or out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < M or out.shape[1] < n_out:
            raise capi.TcavtError(f"gemm_mx8.out: 2-D GPU tensor of at least ({M}, {n_out}) with unit column stride required")
        args.C, args.ldc, args.out_dtype = out.data_ptr(), out.stride(0), _DT[out.dtype]
    for k, v in fields.items():  # (tensors and scalars mixed: not capi.bind's case)
        setattr(args, k, v.data_ptr() if torch.is_tensor(v) else v)
    check(lib().tcavt_gemm_mx8(ctypes.byref(args), stream_ptr()), "tcavt_gemm_mx8")
    return out


def norm_npart(M, N, K):
    """Partial sums of squares per row that a NORM_OUT product [M, N] over K writes (tcavt_norm_npart)."""
    return int(lib().tcavt_norm_npart(int(M), int(N), int(K)))


def embed_fuse(table, ids, img, vis_mod, txt_mod, h, bad_flag, h16=None, part=None, npart=None, stream_scale=1.0):
    """h16 / part (both or neither): the 16-bit copy of h and its rows' partial sums of squares [rows, H / 64] -- the
    inputs of the first decoder layer's fused RMSNorm (tcavt_llama_stack_forward).  stream_scale: h16 and part hold
    stream_scale * h (tcavt_llama_stack_args.stream_scale)."""
    _req16(table, "embed.table")
    _req(ids, torch.int64, "embed.ids")
    _req(img, torch.float32, "embed.img")
    B, Lt = ids.shape
    V, H = table.shape
    Nq = img.numel() // (B * H)
    _need(img, B * Nq * H, "embed.img")
    if h is None and h16 is None:
        raise capi.TcavtError("embed: h (fp32 stream) or h16 (16-bit residual stream) required")
    if h is not None:
        _req(h, torch.float32, "embed.h")
        _need(h, B * (Nq + Lt) * H, "embed.h")
    _need(vis_mod, H, "embed.vis_mod")
    _need(txt_mod, H, "embed.txt_mod")
    _need(bad_flag, 1, "embed.bad_flag")
    if (h16 is None) != (part is None):
        raise capi.TcavtError("embed.h16 and embed.part go together")
    if h16 is not None:
        _req16(h16, "embed.h16", like=table)
        _req(part, torch.float32, "embed.part")
        npart = int(npart or H // 64)
        _need(h16, B * (Nq + Lt) * H, "embed.h16")
        _need(part, B * (Nq + Lt) * npart, "embed.part")
    check(lib().tcavt_embed_fuse(ptr(table), ptr(ids), ptr(img), ptr(vis_mod), ptr(txt_mod), ptr(h), B, Nq, Lt, H,
                                 V, ptr(bad_flag), _DT[table.dtype], ptr(h16), ptr(part), npart if h16 is not None else 0, float(stream_scale),
                                 stream_ptr()),
          "tcavt_embed_fuse")


def mask_to_kvlen(mask, Nq, kv_len, flag):
    _req(mask, torch.int64, "mask_to_kvlen.mask")
    B, Lt = mask.shape
    _need(kv_len, B, "mask_to_kvlen.kv_len")
    _need(flag, 1, "mask_to_kvlen.flag")
    check(lib().tcavt_mask_to_kvlen(ptr(mask), B, Lt, Nq, ptr(kv_len), ptr(flag), stream_ptr()),
          "tcavt_mask_to_kvlen")


def attn_causal_gqa(qkv, out, kv_len, B, L, nq, nkv, scale, lse=None):
    """lse (optional, fp32 [B, nq, L]): receives the log-sum-exp of every query row's scaled scores (for attn_bwd_scores)."""
    _req16(qkv, "attn.qkv")
    _req16(out, "attn.out", like=qkv)
    _req(kv_len, torch.int32, "attn.kv_len")
    _need(qkv, B * L * (nq + 2 * nkv) * 64, "attn.qkv")
    _need(out, B * L * nq * 64, "attn.out")
    _need(kv_len, B, "attn.kv_len")
    if lse is not None:
        _req(lse, torch.float32, "attn.lse")
        _need(lse, B * nq * L, "attn.lse")
    check(lib().tcavt_attn_causal_gqa_lse(ptr(qkv), ptr(out), ptr(lse) if lse is not None else None, ptr(kv_len), B, L, nq, nkv,
                                          scale, _DT[qkv.dtype], stream_ptr()), "tcavt_attn_causal_gqa")


ATTN_RESIDENT_MAX_L = 544  # tcavt_attn_causal_gqa(_lse): K and V^T of a (sample, kv head) resident in LDS
ATTN_STREAM_MAX_L = 2048   # TCAVT_ATTN_STREAM_MAX_L: tcavt_attn_causal_gqa_stream, tcavt_attn_bwd_stream


def attn_causal_gqa_stream(qkv, out, kv_len, B, L, nq, nkv, scale, lse=None):
    """attn_causal_gqa with K and V^T streamed through LDS in chunks of 256 keys (tcavt_attn_causal_gqa_stream): the same
    arguments, semantics and lse convention, 1 <= L <= ATTN_STREAM_MAX_L.  The decoder stack takes it for L > 544."""
    _req16(qkv, "attn_stream.qkv")
    _req16(out, "attn_stream.out", like=qkv)
    _req(kv_len, torch.int32, "attn_stream.kv_len")
    _need(qkv, B * L * (nq + 2 * nkv) * 64, "attn_stream.qkv")
    _need(out, B * L * nq * 64, "attn_stream.out")
    _need(kv_len, B, "attn_stream.kv_len")
    if lse is not None:
        _req(lse, torch.float32, "attn_stream.lse")
        _need(lse, B * nq * L, "attn_stream.lse")
    check(lib().tcavt_attn_causal_gqa_stream(ptr(qkv), ptr(out), ptr(lse) if lse is not None else None, ptr(kv_len), B, L, nq,
                                             nkv, scale, _DT[qkv.dtype], stream_ptr()), "tcavt_attn_causal_gqa_stream")


def mha(q, k, v, out, B, Lq, Lk, nh, dh, scale, key_len=None, ldq=None, ldk=None, ldv=None, ldo=None, dropout=None):
    """q/k/v may be column slices of wider row-major buffers: pass the slice's data_ptr tensor and ld."""
    in_dt, out_dt = _DT[q.dtype], _DT[out.dtype]
    if k.dtype != q.dtype or v.dtype != q.dtype:
        raise capi.TcavtError("mha: q, k, v must share a dtype")
    lq, lk, lv, lo = (ldq or q.stride(-2)), (ldk or k.stride(-2)), (ldv or v.stride(-2)), (ldo or out.stride(-2))
    E = nh * dh
    for t, rows, ld, nm in ((q, B * Lq, lq, "q"), (k, B * Lk, lk, "k"), (v, B * Lk, lv, "v"), (out, B * Lq, lo, "out")):
        if ld < E:
            raise capi.TcavtError(f"mha.{nm}: leading dimension {ld} < nh*dh = {E}")
        avail = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
        if avail < (rows - 1) * ld + E:
            raise capi.TcavtError(f"mha.{nm}: buffer too small for {rows} rows of stride {ld}")
    _need(key_len, B, "mha.key_len")
    check(lib().tcavt_mha(ptr(q), ldq if ldq else q.stride(-2), ptr(k), ldk if ldk else k.stride(-2), ptr(v),
                          ldv if ldv else v.stride(-2), ptr(out), ldo if ldo else out.stride(-2), ptr(key_len), B,
                          Lq, Lk, nh, dh, scale, in_dt, out_dt, *_drop(dropout), stream_ptr()), "tcavt_mha")


def gemm_f32(a, w, out=None, bias=None, relu=False, residual=None, dropout=None):
    _req(a, torch.float32, "gemm_f32.a")
    _req(w, torch.float32, "gemm_f32.w")
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    flags = (EPI_BIAS if bias is not None else 0) | (EPI_RELU if relu else 0) | (
        EPI_RESIDUAL if residual is not None else 0)
    if w.shape[1] != K or out.shape[0] < M or out.shape[1] < N:
        raise capi.TcavtError(f"gemm_f32: shape mismatch a{tuple(a.shape)} w{tuple(w.shape)} out{tuple(out.shape)}")
    if bias is not None:
        _need(bias, N, "gemm_f32.bias")
    if residual is not None and (residual.shape[0] < M or residual.shape[1] < N):
        raise capi.TcavtError("gemm_f32.residual: smaller than (M, N)")
    check(lib().tcavt_gemm_f32(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(residual),
                               residual.stride(0) if residual is not None else 0, ptr(out), out.stride(0), M, N, K,
                               flags, *_drop(dropout), stream_ptr()), "tcavt_gemm_f32")
    return out


def poly_embed(polygon, w_in, b_in, pos, out):
    B, P, _ = polygon.shape
    D = w_in.shape[0]
    _need(pos, P * D, "poly_embed.pos")
    _need(out, B * P * D, "poly_embed.out")
    check(lib().tcavt_poly_embed(ptr(polygon), ptr(w_in), ptr(b_in), ptr(pos), ptr(out), B, P, D, stream_ptr()),
          "tcavt_poly_embed")


def masked_mean(enc, lens, out, B, P, D):
    _need(enc, B * P * D, "masked_mean.enc")
    _need(lens, B, "masked_mean.lens")
    _need(out, B * D, "masked_mean.out")
    check(lib().tcavt_masked_mean(ptr(enc), ptr(lens), ptr(out), B, P, D, stream_ptr()), "tcavt_masked_mean")


def ltsf_front(x, conv_w, conv_b, enc_w, enc_b, pos, out, B, C, T, xp_tok=None):
    _need(xp_tok, B * T * C, "ltsf_front.xp_tok")
    for t, n, nm in ((x, B * 2 * T, "x"), (conv_w, C * 2, "conv_w"), (conv_b, C, "conv_b"), (enc_w, C * T * T, "enc_w"),
                     (enc_b, C * T, "enc_b"), (pos, C * T, "pos"), (out, B * T * C, "out")):
        _need(t, n, "ltsf_front." + nm)
    check(lib().tcavt_ltsf_front(ptr(x), ptr(conv_w), ptr(conv_b), ptr(enc_w), ptr(enc_b), ptr(pos), ptr(out),
                                 ptr(xp_tok), B, C, T, stream_ptr()), "tcavt_ltsf_front")


def ltsf_decode(e_tok, dec_w, dec_b, lane_adj, out, B, C, T, To):
    for t, n, nm in ((e_tok, B * T * C, "e_tok"), (dec_w, C * To * T, "dec_w"), (dec_b, C * To, "dec_b"),
                     (lane_adj, B * C * To, "lane_adj"), (out, B * C * To, "out")):
        _need(t, n, "ltsf_decode." + nm)
    check(lib().tcavt_ltsf_decode(ptr(e_tok), ptr(dec_w), ptr(dec_b), ptr(lane_adj), ptr(out), B, C, T, To,
                                  stream_ptr()), "tcavt_ltsf_decode")


def transpose_ct(x, out_f32, out_bf16, B, C, To):
    for t, nm in ((x, "x"), (out_f32, "out_f32"), (out_bf16, "out_bf16")):
        _need(t, B * C * To, "transpose_ct." + nm)
    _req16(out_bf16, "transpose_ct.out_bf16")
    check(lib().tcavt_transpose_ct(ptr(x), ptr(out_f32), ptr(out_bf16), B, C, To,
                                   _DT[out_bf16.dtype] if out_bf16 is not None else BF16, stream_ptr()), "tcavt_transpose_ct")


def out_head(fused, w, bias, x, out, B, To, C, F, T, add_last=True):
    for t, n, nm in ((fused, B * To * C, "fused"), (w, F * C, "w"), (bias, F, "bias"), (x, B * F * T, "x"),
                     (out, B * F * To, "out")):
        _need(t, n, "out_head." + nm)
    check(lib().tcavt_out_head(ptr(fused), ptr(w), ptr(bias), ptr(x), ptr(out), B, To, C, F, T, int(add_last),
                               stream_ptr()),
          "tcavt_out_head")


def traj_metrics(pred, gt, norm_stat, sums, argmin, per_sample, B, K, To):
    for t, n, nm in ((pred, B * K * 2 * To, "pred"), (gt, B * 2 * To, "gt"), (norm_stat, B * 4, "norm_stat"),
                     (sums, 5, "sums"), (argmin, B * 3, "argmin"), (per_sample, B * 3, "per_sample")):
        _need(t, n, "traj_metrics." + nm)
    check(lib().tcavt_traj_metrics(ptr(pred), ptr(gt), ptr(norm_stat), ptr(sums), ptr(argmin), ptr(per_sample), B,
                                   K, To, stream_ptr()), "tcavt_traj_metrics")


# ----------------------------------------------------------------------------------------------
# training-step kernels (include/tcavt.h, second half)
# ----------------------------------------------------------------------------------------------
def gemm_f32_strided(a, rsA, csA, w, rsW, csW, out, M, N, K, bias=None, relu=False, residual=None, accumulate=False):
    for t, rs, cs, rows, nm in ((a, rsA, csA, M, "a"), (w, rsW, csW, N, "w")):
        if _avail(t) < (rows - 1) * rs + (K - 1) * cs + 1:
            raise capi.TcavtError(f"gemm_f32_strided.{nm}: buffer too small")
    if _avail(out) < (M - 1) * out.stride(0) + N:
        raise capi.TcavtError("gemm_f32_strided.out: buffer too small")
    flags = (EPI_BIAS if bias is not None else 0) | (EPI_RELU if relu else 0) | (
        EPI_RESIDUAL if residual is not None else 0) | (capi.EPI_ACCUM if accumulate else 0)
    ws = None  # split-K partial sums (added in a fixed order), when the launcher may split: few output tiles, long K
    if -(-M // 64) * -(-N // 64) < 128 and K >= 512 and not relu:
        ws = torch.empty(min(8, K // 256) * M * N, dtype=torch.float32, device=out.device)
    check(lib().tcavt_gemm_f32_strided(ptr(a), rsA, csA, ptr(w), rsW, csW, ptr(bias), ptr(residual),
                                       residual.stride(0) if residual is not None else 0, ptr(out), out.stride(0), M, N,
                                       K, flags, ptr(ws), ws.numel() if ws is not None else 0, stream_ptr()),
          "tcavt_gemm_f32_strided")
    return out


def transpose16(x, out, rows, cols, rows_pad, ld_in=None, ld_out=None, batch=1, s_in=0, s_out=0):
    """out[c][r] = x[r][c] (16-bit), zero-filled for r in [rows, rows_pad); batched with strides.  An fp16 source with a
    bf16 destination is converted on the way (forward activations entering a gradient-side contraction)."""
    ld_in = ld_in or x.stride(-2)
    ld_out = ld_out or out.stride(-2)
    if _avail(x) < (batch - 1) * s_in + (rows - 1) * ld_in + cols or \
            _avail(out) < (batch - 1) * s_out + (cols - 1) * ld_out + rows_pad:
        raise capi.TcavtError("transpose16: buffer too small")
    if x.element_size() != 2 or out.element_size() != 2:
        raise capi.TcavtError("transpose16: 16-bit tensors only")
    if x.dtype != out.dtype and not (x.dtype == torch.float16 and out.dtype == torch.bfloat16):
        raise capi.TcavtError("transpose16: same 16-bit type on both sides, or fp16 -> bf16")
    check(lib().tcavt_transpose16(ptr(x), ld_in, ptr(out), ld_out, rows, cols, rows_pad, batch, s_in, s_out,
                                  int(x.dtype != out.dtype), stream_ptr()), "tcavt_transpose16")
    return out


def transpose_f32_bf16(x, out, rows, cols, rows_pad):
    _req(x, torch.float32, "transpose_f32_bf16.x")
    if _avail(x) < (rows - 1) * x.stride(0) + cols or _avail(out) < (cols - 1) * out.stride(0) + rows_pad:
        raise capi.TcavtError("transpose_f32_bf16: buffer too small")
    check(lib().tcavt_transpose_f32_bf16(ptr(x), x.stride(0), ptr(out), out.stride(0), rows, cols, rows_pad,
                                         stream_ptr()), "tcavt_transpose_f32_bf16")
    return out


def colsum(g, out, M, N, accumulate=False):
    _need(out, N, "colsum.out")
    if _avail(g) < (M - 1) * g.stride(0) + N:
        raise capi.TcavtError("colsum.g: buffer too small")
    ws = torch.empty(-(-M // 128) * N, dtype=torch.float32, device=g.device)  # per-block partial sums (fixed-order reduce)
    check(lib().tcavt_colsum(ptr(g), g.stride(0), _DT[g.dtype], ptr(out), M, N, int(accumulate), ptr(ws), ws.numel(),
                             stream_ptr()), "tcavt_colsum")


def relu_bwd(g, y):
    _req(g, torch.float32, "relu_bwd.g")
    _need(y, g.numel(), "relu_bwd.y")
    check(lib().tcavt_relu_bwd(ptr(g), ptr(y), _DT[y.dtype], g.numel(), stream_ptr()), "tcavt_relu_bwd")


def add_inplace(a, b):
    _req(a, torch.float32, "add_inplace.a")
    _req(b, torch.float32, "add_inplace.b")
    _need(b, a.numel(), "add_inplace.b")
    check(lib().tcavt_add_inplace(ptr(a), ptr(b), a.numel(), stream_ptr()), "tcavt_add_inplace")


def silu_mul_bwd(gu, g_act, g_gu):
    """d(silu(gate) * up) in the interleaved gate|up layout (layout.interleave_gate_up)."""
    M, I = g_act.shape
    for t, n, nm in ((gu, 2 * M * I, "gu"), (g_act, M * I, "g_act"), (g_gu, 2 * M * I, "g_gu")):
        _req(t, gu.dtype, "silu_mul_bwd." + nm)  # one 16-bit type for all three (bf16, or fp16 with scaled gradients)
        _need(t, n, "silu_mul_bwd." + nm)
    check(lib().tcavt_silu_mul_bwd(ptr(gu), ptr(g_act), ptr(g_gu), M, I, _DT16(gu), stream_ptr()), "tcavt_silu_mul_bwd")


def _DT16(t):
    if t.dtype not in _H16:
        raise capi.TcavtError(f"16-bit tensor (fp16 / bf16) required, got {t.dtype}")
    return _DT[t.dtype]


def grad_scale_pick(g_a, g_b, scale, scratch, target=256.0, backoff=None):
    """scale[0] = 2^k with max|g_a, g_b| * 2^k in [target / 2, target], scale[1] = its inverse -- on the device
    (tcavt_grad_scale_pick).  scratch: one zero-initialised int32."""
    n = g_a.numel()
    if g_b is not None and (g_b.dtype != g_a.dtype or g_b.numel() != n):
        raise capi.TcavtError("grad_scale_pick: g_b must match g_a")
    _req(scale, torch.float32, "grad_scale_pick.scale")
    _need(scale, 2, "grad_scale_pick.scale")
    if scratch.dtype != torch.int32 or scratch.numel() < 1:
        raise capi.TcavtError("grad_scale_pick.scratch: int32 [1] required")
    if backoff is not None:
        _req(backoff, torch.int32, "grad_scale_pick.backoff")
    check(lib().tcavt_grad_scale_pick(ptr(g_a), ptr(g_b) if g_b is not None else None, n, _DT16(g_a), float(target), ptr(scale),
                                      ptr(scratch), ptr(backoff), stream_ptr()), "tcavt_grad_scale_pick")


def rmsnorm_bwd(x, gamma, gy, gx, eps, gy2=None, accumulate=False, gx_bf16=None, gy_scale=None):
    M, H = x.shape
    if x.dtype not in (torch.float32,) + _H16:
        raise capi.TcavtError("rmsnorm_bwd.x: fp32 or a 16-bit residual stream required")
    _need(x, M * H, "rmsnorm_bwd.x")
    _req(gx, torch.float32, "rmsnorm_bwd.gx")
    _req(gamma, torch.float32, "rmsnorm_bwd.gamma")
    _need(gamma, H, "rmsnorm_bwd.gamma")
    _need(gx, M * H, "rmsnorm_bwd.gx")
    for t, nm in ((gy, "gy"), (gy2, "gy2"), (gx_bf16, "gx_bf16")):
        if t is not None:
            _DT16(t)
            _need(t, M * H, "rmsnorm_bwd." + nm)
    if gy2 is not None and gy2.dtype != gy.dtype:
        raise capi.TcavtError("rmsnorm_bwd: gy and gy2 must have one 16-bit type")
    if gy_scale is not None:
        _req(gy_scale, torch.float32, "rmsnorm_bwd.gy_scale")
    check(lib().tcavt_rmsnorm_bwd(ptr(x), ptr(gamma), ptr(gy), ptr(gy2) if gy2 is not None else None, eps, ptr(gx),
                                  ptr(gx_bf16) if gx_bf16 is not None else None, int(accumulate), M, H, _DT16(gy),
                                  _DT16(gx_bf16) if gx_bf16 is not None else 0,
                                  ptr(gy_scale) if gy_scale is not None else None, _DT[x.dtype], stream_ptr()),
          "tcavt_rmsnorm_bwd")


def rope_bwd_pack(g32, out, cos, sin, rope_cols, L):
    M, ncols = g32.shape
    _req(g32, torch.float32, "rope_bwd_pack.g32")
    _need(out, M * ncols, "rope_bwd_pack.out")
    _need(cos, L * 32, "rope_bwd_pack.cos")
    _need(sin, L * 32, "rope_bwd_pack.sin")
    check(lib().tcavt_rope_bwd_pack(ptr(g32), ptr(out), ptr(cos), ptr(sin), M, ncols, rope_cols, L, _DT16(out), stream_ptr()),
          "tcavt_rope_bwd_pack")


def attn_causal_gqa_bwd(qkv, dO, g32, kv_len, B, T, nq, nkv, scale):
    """Backward of attn_causal_gqa; g32 (fp32, q|k|v layout) must be zeroed by the caller."""
    ncols = (nq + 2 * nkv) * 64
    _req(qkv, torch.bfloat16, "attn_causal_gqa_bwd.qkv")
    _req(dO, torch.bfloat16, "attn_causal_gqa_bwd.dO")
    _req(g32, torch.float32, "attn_causal_gqa_bwd.g32")
    _need(qkv, B * T * ncols, "attn_causal_gqa_bwd.qkv")
    _need(g32, B * T * ncols, "attn_causal_gqa_bwd.g32")
    _need(dO, B * T * nq * 64, "attn_causal_gqa_bwd.dO")
    _need(kv_len, B, "attn_causal_gqa_bwd.kv_len")
    check(lib().tcavt_attn_causal_gqa_bwd(ptr(qkv), ptr(dO), ptr(g32), ptr(kv_len), B, T, nq, nkv, 64, scale,
                                          stream_ptr()), "tcavt_attn_causal_gqa_bwd")


def causal_softmax_bwd_rows(S, dP, P, dS, kv_len, B, T, Tp, nq, scale):
    rows = B * nq * T
    for t, dt, nm in ((S, torch.float32, "S"), (dP, torch.float32, "dP"), (P, torch.bfloat16, "P"), (dS, torch.bfloat16, "dS")):
        _req(t, dt, "causal_softmax_bwd_rows." + nm)
        _need(t, rows * Tp, "causal_softmax_bwd_rows." + nm)
    _need(kv_len, B, "causal_softmax_bwd_rows.kv_len")
    check(lib().tcavt_causal_softmax_bwd_rows(ptr(S), ptr(dP), ptr(P), ptr(dS), ptr(kv_len), B, T, Tp, nq, scale,
                                              stream_ptr()), "tcavt_causal_softmax_bwd_rows")


def causal_softmax_bwd_tiles(S, dP, dS, PT, dST, kv_len, B, T, Tp, nq, scale):
    """Tiled form of causal_softmax_bwd_rows: dS row-major plus P^T, dS^T; the outputs must have been zero-initialised
    once (blocks above the causal diagonal are never written)."""
    rows = B * nq * T
    for t, dt, n, nm in ((S, torch.float32, rows * Tp, "S"), (dP, torch.float32, rows * Tp, "dP"),
                         (dS, torch.bfloat16, rows * Tp, "dS"), (PT, torch.bfloat16, B * nq * Tp * Tp, "PT"),
                         (dST, torch.bfloat16, B * nq * Tp * Tp, "dST")):
        _req(t, dt, "causal_softmax_bwd_tiles." + nm)
        _need(t, n, "causal_softmax_bwd_tiles." + nm)
    _need(kv_len, B, "causal_softmax_bwd_tiles.kv_len")
    check(lib().tcavt_causal_softmax_bwd_tiles(ptr(S), ptr(dP), ptr(dS), ptr(PT), ptr(dST), ptr(kv_len), B, T, Tp, nq, scale,
                                               stream_ptr()), "tcavt_causal_softmax_bwd_tiles")


def attn_bwd_dkv(qkv, dO, stats, g32, kv_len, B, T, Tp, nq, nkv, scale):
    """dK, dV of the causal GQA attention (key-major MFMA kernel) into the k / v columns of g32 (fp32, q|k|v layout)."""
    ncols = (nq + 2 * nkv) * 64
    for t, dt, n, nm in ((qkv, qkv.dtype, B * T * ncols, "qkv"), (dO, qkv.dtype, B * T * nq * 64, "dO"),
                         (stats, torch.float32, B * nq * T * 4, "stats"), (g32, torch.float32, B * T * ncols, "g32")):
        if t.dtype != dt or (not t.is_cuda and not _ALLOW_CPU) or _avail(t) < n:
            raise capi.TcavtError(f"attn_bwd_dkv.{nm}: {dt} GPU buffer with {n} elements required")
    _need(kv_len, B, "attn_bwd_dkv.kv_len")
    check(lib().tcavt_attn_bwd_dkv(ptr(qkv), ptr(dO), ptr(stats), ptr(g32), ptr(kv_len), B, T, Tp, nq, nkv, 64, scale,
                                   _DT16(qkv), stream_ptr()), "tcavt_attn_bwd_dkv")


def attn_bwd_scores(qkv, dO, dS, PT, dST, kv_len, B, T, Tp, nq, nkv, scale, dQ=None, stats=None, lse=None, att=None):
    """Scores + softmax backward in one kernel (MFMA inside): P^T, dS^T (zero-initialised once), plus dQ = dS K (fp32
    [B*T, >= nq*64], any leading dimension) computed in place and / or the row-major dS for an external dQ product.
    lse (fp32 [B*nq*T]) + att (the forward's output, 16-bit [B*T, nq*64]), from attn_causal_gqa(..., lse=...): the row
    statistics come from the forward and the kernel sweeps the keys once instead of twice."""
    rows, ncols = B * nq * T, (nq + 2 * nkv) * 64
    if dQ is not None:
        if dQ.dtype != torch.float32 or dQ.stride(-1) != 1 or _avail(dQ) < (B * T - 1) * dQ.stride(0) + nq * 64:
            raise capi.TcavtError("attn_bwd_scores.dQ: fp32 [B*T, >= nq*64] required")
    for t, n, nm in ((qkv, B * T * ncols, "qkv"), (dO, B * T * nq * 64, "dO"), (dS, rows * Tp, "dS"),
                     (PT, B * nq * Tp * Tp, "PT"), (dST, B * nq * Tp * Tp, "dST")):
        if t is None and ((nm == "dS" and dQ is not None) or (nm in ("PT", "dST") and stats is not None)):
            continue
        if t.dtype != qkv.dtype or t.dtype not in _H16 or (not t.is_cuda and not _ALLOW_CPU):
            raise capi.TcavtError(f"attn_bwd_scores.{nm}: 16-bit GPU tensor of the type of qkv required")
        if _avail(t) < n:
            raise capi.TcavtError(f"attn_bwd_scores.{nm}: buffer too small")
    _need(kv_len, B, "attn_bwd_scores.kv_len")
    if stats is not None:
        _req(stats, torch.float32, "attn_bwd_scores.stats")
        _need(stats, rows * 4, "attn_bwd_scores.stats")
    if (lse is None) != (att is None):
        raise capi.TcavtError("attn_bwd_scores: lse and att come together")
    if lse is not None:
        _req(lse, torch.float32, "attn_bwd_scores.lse")
        _need(lse, rows, "attn_bwd_scores.lse")
        if att.dtype != qkv.dtype or not att.is_contiguous() or _avail(att) < B * T * nq * 64:
            raise capi.TcavtError("attn_bwd_scores.att: contiguous 16-bit [B*T, nq*64] of the type of qkv required")
    opt = lambda t: ptr(t) if t is not None else None
    check(lib().tcavt_attn_bwd_scores(ptr(qkv), ptr(dO), opt(dS), opt(PT), opt(dST), opt(dQ),
                                      dQ.stride(0) if dQ is not None else 0, opt(stats), ptr(kv_len), B, T, Tp, nq, nkv, 64,
                                      scale, _DT16(qkv), opt(lse), opt(att), stream_ptr()), "tcavt_attn_bwd_scores")


def attn_bwd_resident_ok(T, nq, nkv):
    """Shapes the two-launch resident form of the attention backward serves (T <= 256, 16 % (nq / nkv) == 0)."""
    return bool(lib().tcavt_attn_bwd_resident_ok(T, nq, nkv))


def attn_bwd_resident(qkv, dO, att, lse, g_qkv, stats, cos, sin, kv_len, B, T, nq, nkv, scale):
    """The whole causal GQA attention backward in two launches (tcavt_attn_bwd_resident): g_qkv 16-bit [B*T, (nq+2nkv)*64]
    = gradient of the projections' outputs, RoPE undone; att / lse from attn_causal_gqa(..., lse=...)."""
    return _attn_bwd_two_launch("attn_bwd_resident", qkv, dO, att, lse, g_qkv, stats, cos, sin, kv_len, B, T, nq, nkv, scale)


def _attn_bwd_two_launch(name, qkv, dO, att, lse, g_qkv, stats, cos, sin, kv_len, B, T, nq, nkv, scale):
    ncols = (nq + 2 * nkv) * 64
    for t, n, nm in ((qkv, B * T * ncols, "qkv"), (dO, B * T * nq * 64, "dO"), (att, B * T * nq * 64, "att"),
                     (g_qkv, B * T * ncols, "g_qkv")):
        if t.dtype != qkv.dtype or t.dtype not in _H16 or not t.is_contiguous() or (not t.is_cuda and not _ALLOW_CPU):
            raise capi.TcavtError(f"{name}.{nm}: contiguous 16-bit GPU tensor of the type of qkv required")
        if _avail(t) < n:
            raise capi.TcavtError(f"{name}.{nm}: buffer too small")
    for t, n, nm in ((lse, B * nq * T, "lse"), (stats, B * nq * T * 4, "stats"), (cos, T * 32, "cos"), (sin, T * 32, "sin")):
        _req(t, torch.float32, f"{name}.{nm}")
        _need(t, n, f"{name}.{nm}")
    _need(kv_len, B, f"{name}.kv_len")
    check(getattr(lib(), "tcavt_" + name)(ptr(qkv), ptr(dO), ptr(att), ptr(lse), ptr(g_qkv), ptr(stats), ptr(cos), ptr(sin),
                                          ptr(kv_len), B, T, nq, nkv, 64, scale, _DT16(qkv), stream_ptr()), "tcavt_" + name)
    return g_qkv


def attn_bwd_long_ok(T, nq, nkv):
    """Shapes the dispatch hands to the chunked form of the attention backward (256 < T <= 544, 16 % (nq / nkv) == 0)."""
    return bool(lib().tcavt_attn_bwd_long_ok(T, nq, nkv))


def attn_bwd_long(qkv, dO, att, lse, g_qkv, stats, cos, sin, kv_len, B, T, nq, nkv, scale):
    """attn_bwd_resident in chunks of 256 keys / queries (tcavt_attn_bwd_long): same arguments and outputs, any T <= 544."""
    return _attn_bwd_two_launch("attn_bwd_long", qkv, dO, att, lse, g_qkv, stats, cos, sin, kv_len, B, T, nq, nkv, scale)


def attn_bwd_stream_ok(T, nq, nkv):
    """Shapes the dispatch hands to the chunked backward beyond 544 (544 < T <= 2048, 16 % (nq / nkv) == 0)."""
    return bool(lib().tcavt_attn_bwd_stream_ok(T, nq, nkv))


def attn_bwd_stream(qkv, dO, att, lse, g_qkv, stats, cos, sin, kv_len, B, T, nq, nkv, scale):
    """attn_bwd_long under the cap of the streaming forward (tcavt_attn_bwd_stream): same arguments and outputs, any T <= 2048."""
    return _attn_bwd_two_launch("attn_bwd_stream", qkv, dO, att, lse, g_qkv, stats, cos, sin, kv_len, B, T, nq, nkv, scale)


def gqa_rope_bwd_pack(G3, out, cos, sin, nq, nkv, L):
    M = G3.shape[0]
    _req(G3, torch.float32, "gqa_rope_bwd_pack.G3")
    _req(out, torch.bfloat16, "gqa_rope_bwd_pack.out")
    _need(G3, M * 3 * nq * 64, "gqa_rope_bwd_pack.G3")
    _need(out, M * (nq + 2 * nkv) * 64, "gqa_rope_bwd_pack.out")
    _need(cos, L * 32, "gqa_rope_bwd_pack.cos")
    _need(sin, L * 32, "gqa_rope_bwd_pack.sin")
    check(lib().tcavt_gqa_rope_bwd_pack(ptr(G3), ptr(out), ptr(cos), ptr(sin), M, nq, nkv, 64, L, stream_ptr()),
          "tcavt_gqa_rope_bwd_pack")


def layernorm_bwd(x, gamma, gy, gx, ggamma, gbeta, eps=1e-5):
    M, D = x.shape
    for t, n, nm in ((gamma, D, "gamma"), (gy, M * D, "gy"), (gx, M * D, "gx"), (ggamma, D, "ggamma"), (gbeta, D, "gbeta")):
        _req(t, torch.float32, "layernorm_bwd." + nm)
        _need(t, n, "layernorm_bwd." + nm)
    ws = torch.empty(-(-M // 16) * 2 * D, dtype=torch.float32, device=x.device)  # per-block partial sums (fixed-order reduce)
    check(lib().tcavt_layernorm_bwd(ptr(x), ptr(gamma), ptr(gy), eps, ptr(gx), ptr(ggamma), ptr(gbeta), M, D,
                                    ptr(ws), ws.numel(), stream_ptr()), "tcavt_layernorm_bwd")


def mha_bwd(q, k, v, go, gq, gk, gv, B, Lq, Lk, nh, dh, scale, key_len=None, ldq=None, ldk=None, ldv=None, ldo=None,
            ldg=None, dropout=None):
    E = nh * dh
    lq, lk, lv, lo, lg = (ldq or q.stride(-2)), (ldk or k.stride(-2)), (ldv or v.stride(-2)), (ldo or go.stride(-2)), (
        ldg or gq.stride(-2))
    for t, rows, ld, nm in ((q, B * Lq, lq, "q"), (k, B * Lk, lk, "k"), (v, B * Lk, lv, "v"), (go, B * Lq, lo, "go"),
                            (gq, B * Lq, lg, "gq"), (gk, B * Lk, lg, "gk"), (gv, B * Lk, lg, "gv")):
        if t.dtype != torch.float32 or _avail(t) < (rows - 1) * ld + E:
            raise capi.TcavtError(f"mha_bwd.{nm}: fp32 buffer with {rows} rows of stride {ld} required")
    _need(key_len, B, "mha_bwd.key_len")
    check(lib().tcavt_mha_bwd(ptr(q), lq, ptr(k), lk, ptr(v), lv, ptr(go), lo, ptr(gq), ptr(gk), ptr(gv), lg,
                              ptr(key_len), B, Lq, Lk, nh, dh, scale, *_drop(dropout), stream_ptr()), "tcavt_mha_bwd")


def softmax_bwd_rows(p_f16, dP, dS, scale, rows, n_valid, n_out, ldp, ldd, lds):
    if p_f16.dtype != torch.float16 or dP.dtype != torch.float32 or dS.dtype != torch.bfloat16:
        raise capi.TcavtError("softmax_bwd_rows: P fp16, dP fp32, dS bf16 required")
    if _avail(p_f16) < (rows - 1) * ldp + n_valid or _avail(dP) < (rows - 1) * ldd + n_valid or \
            _avail(dS) < (rows - 1) * lds + n_out:
        raise capi.TcavtError("softmax_bwd_rows: buffer too small")
    check(lib().tcavt_softmax_bwd_rows(ptr(p_f16), ldp, ptr(dP), ldd, ptr(dS), lds, scale, rows, n_valid, n_out,
                                       stream_ptr()), "tcavt_softmax_bwd_rows")


def mse_grad(pred, gt, norm_stat, g, B, To):
    for t, n, nm in ((pred, B * 2 * To, "pred"), (gt, B * 2 * To, "gt"), (norm_stat, B * 4, "norm_stat"), (g, B * 2 * To, "g")):
        _req(t, torch.float32, "mse_grad." + nm)
        _need(t, n, "mse_grad." + nm)
    check(lib().tcavt_mse_grad(ptr(pred), ptr(gt), ptr(norm_stat), ptr(g), B, To, stream_ptr()), "tcavt_mse_grad")


def mse_grad_seeded(pred, gt, norm_stat, g, B, To, g_loss=None, g_pred=None):
    """g = g_loss[0] * mse_grad(pred, gt, norm_stat) + g_pred (autograd's seeds: g_loss a device fp32 scalar, read on the
    device; g_pred [B, 2, To]).  A None term is absent; both None is refused.  g_loss = 1, g_pred None: mse_grad's bits."""
    if g_loss is None and g_pred is None:
        raise capi.TcavtError("mse_grad_seeded: g_loss and g_pred are both None")
    checks = [(g, B * 2 * To, "g"), (g_loss, 1, "g_loss"), (g_pred, B * 2 * To, "g_pred")]
    if g_loss is not None:
        checks += [(pred, B * 2 * To, "pred"), (gt, B * 2 * To, "gt"), (norm_stat, B * 4, "norm_stat")]
    for t, n, nm in checks:
        _req(t, torch.float32, "mse_grad_seeded." + nm)
        _need(t, n, "mse_grad_seeded." + nm)
    if g_loss is None:
        pred = gt = norm_stat = None
    check(lib().tcavt_mse_grad_seeded(ptr(pred), ptr(gt), ptr(norm_stat), ptr(g_loss), ptr(g_pred), ptr(g), B, To,
                                      stream_ptr()), "tcavt_mse_grad_seeded")


def out_head_bwd(g, fused, w, gf, gw, gb, B, To, C, F):
    for t, n, nm in ((g, B * F * To, "g"), (fused, B * To * C, "fused"), (w, F * C, "w"), (gf, B * To * C, "gf"),
                     (gw, F * C, "gw"), (gb, F, "gb")):
        _need(t, n, "out_head_bwd." + nm)
    check(lib().tcavt_out_head_bwd(ptr(g), ptr(fused), ptr(w), ptr(gf), ptr(gw), ptr(gb), B, To, C, F, stream_ptr()),
          "tcavt_out_head_bwd")


def nlinear_bwd(in_tok, W, g, g_strides, gW, gbias, gin_tok, B, C, T, S):
    sb, sc, ss = g_strides
    for t, n, nm in ((in_tok, B * T * C, "in_tok"), (W, C * S * T, "W"), (gW, C * S * T, "gW"), (gbias, C * S, "gbias"),
                     (gin_tok, B * T * C, "gin_tok")):
        _need(t, n, "nlinear_bwd." + nm)
    if _avail(g) < (B - 1) * sb + (C - 1) * sc + (S - 1) * ss + 1:
        raise capi.TcavtError("nlinear_bwd.g: buffer too small")
    check(lib().tcavt_nlinear_bwd(ptr(in_tok), ptr(W), ptr(g), sb, sc, ss, ptr(gW), ptr(gbias), ptr(gin_tok), B, C, T, S,
                                  stream_ptr()), "tcavt_nlinear_bwd")


def conv1x1_bwd(gxp_tok, x, gw, gb, B, C, T, F):
    for t, n, nm in ((gxp_tok, B * T * C, "gxp_tok"), (x, B * F * T, "x"), (gw, C * F, "gw"), (gb, C, "gb")):
        _need(t, n, "conv1x1_bwd." + nm)
    check(lib().tcavt_conv1x1_bwd(ptr(gxp_tok), ptr(x), ptr(gw), ptr(gb), B, C, T, F, stream_ptr()), "tcavt_conv1x1_bwd")


def poly_embed_bwd(g, polygon, gw, gb, gpos, B, P, D):
    for t, n, nm in ((g, B * P * D, "g"), (polygon, B * P * 2, "polygon"), (gw, D * 2, "gw"), (gb, D, "gb"), (gpos, P * D, "gpos")):
        _need(t, n, "poly_embed_bwd." + nm)
    check(lib().tcavt_poly_embed_bwd(ptr(g), ptr(polygon), ptr(gw), ptr(gb), ptr(gpos), B, P, D, stream_ptr()),
          "tcavt_poly_embed_bwd")


def masked_mean_bwd(gemb, lens, genc, B, P, D):
    for t, n, nm in ((gemb, B * D, "gemb"), (lens, B, "lens"), (genc, B * P * D, "genc")):
        _need(t, n, "masked_mean_bwd." + nm)
    check(lib().tcavt_masked_mean_bwd(ptr(gemb), ptr(lens), ptr(genc), B, P, D, stream_ptr()), "tcavt_masked_mean_bwd")


def wgrad_tn(g, g_col0, n, x, out, trans_out=False, rs_part=None, rs_h=0, rs_eps=0.0):
    """out[i, h] += sum_m g[m, g_col0 + i] * x[m, h] (i < n; trans_out: out[h, i]) -- skinny weight gradient without
    transposes (tcavt_wgrad_tn).  g bf16 [M, >= g_col0 + n], x fp16 / bf16 [M, H], out fp32, accumulated into.
    rs_part (fp32 [M, npart], with rs_h, rs_eps): rows of g are scaled by 1 / rms of their token on the way in."""
    if g.dtype not in _H16 or x.dtype not in _H16 or out.dtype != torch.float32 or (g.dtype == torch.float16 and x.dtype != torch.float16):
        raise capi.TcavtError("wgrad_tn: g bf16 with x fp16 / bf16, or g fp16 with x fp16; out fp32")
    M, H = x.shape
    if g.shape[0] < M or g.shape[1] < g_col0 + n or g.stride(1) != 1 or x.stride(1) != 1 or out.stride(1) != 1:
        raise capi.TcavtError("wgrad_tn: operand shapes / strides")
    rows, cols = (H, n) if trans_out else (n, H)
    if out.shape[0] < rows or out.shape[1] < cols:
        raise capi.TcavtError(f"wgrad_tn.out: needs at least ({rows}, {cols})")
    npart = 0
    if rs_part is not None:
        _req(rs_part, torch.float32, "wgrad_tn.rs_part")
        if rs_part.dim() != 2 or rs_part.shape[0] < M or not rs_part.is_contiguous() or rs_h <= 0:
            raise capi.TcavtError("wgrad_tn.rs_part: contiguous fp32 [M, npart] and rs_h > 0 required")
        npart = rs_part.shape[1]
    check(lib().tcavt_wgrad_tn(ptr(g), g.stride(0), int(g_col0), int(n), ptr(x), x.stride(0), _DT[x.dtype], ptr(out), out.stride(0),
                               M, H, int(trans_out), _DT[g.dtype], ptr(rs_part) if rs_part is not None else None, npart, int(rs_h),
                               float(rs_eps), stream_ptr()), "tcavt_wgrad_tn")


def lora_wgrad_a(x16, part, gamma, g_t, dA, eps, dropout=None, site_v=None):
    """dA (fp32 [>= 32, H], accumulated into) of both adapters in one pass over the layer's taped input stream x16 [M, H]:
    rows 0..15 = (g_t[:, :16] * rs)^T drop_q(x16) * gamma, rows 16..31 the v adapter (tcavt_lora_wgrad_a).  part: the
    stream's partial sums of squares [M, npart]; dropout = (p, seed, site_q) with site_v as in lora_down."""
    _req16(x16, "lora_wgrad_a.x16")
    _req16(g_t, "lora_wgrad_a.g_t", like=x16)
    _req(part, torch.float32, "lora_wgrad_a.part")
    _req(gamma, torch.float32, "lora_wgrad_a.gamma")
    _req(dA, torch.float32, "lora_wgrad_a.dA")
    M, H = x16.shape
    if (part.dim() != 2 or part.shape[0] < M or not part.is_contiguous() or g_t.shape[0] < M or g_t.shape[1] != 64
            or not g_t.is_contiguous() or dA.dim() != 2 or dA.shape[0] < 32 or dA.shape[1] < H or dA.stride(1) != 1):
        raise capi.TcavtError("lora_wgrad_a: part [M, npart], g_t [M, 64], dA [>= 32, >= H] required")
    _need(gamma, H, "lora_wgrad_a.gamma")
    p, seed, site = _drop(dropout)
    check(lib().tcavt_lora_wgrad_a(ptr(x16), ptr(part), part.shape[1], float(eps), ptr(gamma), ptr(g_t), ptr(dA), dA.stride(0), M, H,
                                   p, seed, site, site + 1 if site_v is None else int(site_v), _DT16(x16), stream_ptr()),
          "tcavt_lora_wgrad_a")


def clip_grad_norm(g, max_norm, scratch, grad_scale=1.0):
    """In-place g *= grad_scale, then clip of the flat gradient vector to max_norm (torch.nn.utils.clip_grad_norm_
    semantics); scratch: fp32, >= 1026 elements; afterwards scratch[1025] holds the norm of the scaled gradient before
    clipping, scratch[1024] the total factor applied.  grad_scale = 1 / world: clip the data-parallel MEAN gradient."""
    _req(g, torch.float32, "clip_grad_norm.g")
    _req(scratch, torch.float32, "clip_grad_norm.scratch")
    _need(scratch, 1026, "clip_grad_norm.scratch")
    check(lib().tcavt_clip_grad_norm(ptr(g), g.numel(), float(max_norm), float(grad_scale), ptr(scratch), stream_ptr()),
          "tcavt_clip_grad_norm")


def adamw(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    n = p.numel()
    for t, nm in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _req(t, torch.float32, "adamw." + nm)
        _need(t, n, "adamw." + nm)
    check(lib().tcavt_adamw(ptr(p), ptr(g), ptr(m), ptr(v), n, lr, beta1, beta2, eps, weight_decay, int(step),
                            grad_scale, stream_ptr()), "tcavt_adamw")


def adamw_gated(p, g, m, v, lr, beta1, beta2, eps, weight_decay, loss, ctl, grad_scale=1.0, grad_norm=None):
    """AdamW update that the device skips when `loss` (device fp32 scalar) or `grad_norm` (optional device fp32 scalar)
    is not finite (modify_scripts/modify_train.py:1190-1196); the step count lives in ctl (int32[8], device)."""
    n = p.numel()
    for t, nm in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _req(t, torch.float32, "adamw_gated." + nm)
        _need(t, n, "adamw_gated." + nm)
    _req(loss, torch.float32, "adamw_gated.loss")
    _need(loss, 1, "adamw_gated.loss")
    _req(ctl, torch.int32, "adamw_gated.ctl")
    _need(ctl, 8, "adamw_gated.ctl")
    if grad_norm is not None:
        _req(grad_norm, torch.float32, "adamw_gated.grad_norm")
        _need(grad_norm, 1, "adamw_gated.grad_norm")
    check(lib().tcavt_adamw_gated(ptr(p), ptr(g), ptr(m), ptr(v), n, lr, beta1, beta2, eps, weight_decay, grad_scale,
                                  ptr(loss), ptr(grad_norm), ptr(ctl), stream_ptr()), "tcavt_adamw_gated")


# ----------------------------------------------------------------------------------------------
# stage-level entry points (include/tcavt.h "Stage-level entry points")
# ----------------------------------------------------------------------------------------------
def llama_stack_forward(args):
    """args: capi.LlamaStackArgs filled by llama.LlamaWithCrossAttnPEFT (which owns and sizes every buffer it names)."""
    check(lib().tcavt_llama_stack_forward(ctypes.byref(args), stream_ptr()), "tcavt_llama_stack_forward")


def lora_down(x16, a_cat, t, scale, dropout=None, site_v=None):
    """t[:, 0:16] | t[:, 16:32] = scale * dropout_q / dropout_v (x16) . a_cat[0:16 | 16:32]^T in one pass (tcavt_lora_down);
    dropout = (p, seed, site_q) with site_v = site_q + 1 unless given."""
    _req16(x16, "lora_down.x16")
    _req16(a_cat, "lora_down.a_cat", like=x16)
    _req16(t, "lora_down.t", like=x16)
    M, H = x16.shape
    _need(a_cat, 32 * H, "lora_down.a_cat")
    _need(t, M * 64, "lora_down.t")
    p, seed, site = _drop(dropout)
    check(lib().tcavt_lora_down(ptr(x16), ptr(a_cat), ptr(t), M, H, float(scale), p, seed, site,
                                (site + 1) if site_v is None else int(site_v), _DT[x16.dtype], stream_ptr()), "tcavt_lora_down")


def lora_dgrad(g_t, a_qT, a_vT, out, dropout=None, site_v=None):
    """out = mask_q * (g_t[:, :16] . A_q) + mask_v * (g_t[:, 16:32] . A_v) in one pass (tcavt_lora_dgrad); a_qT / a_vT [H, 64]
    with the other adapter's columns zero; dropout = (p, seed, site_q), site_v = site_q + 1 unless given."""
    _req16(g_t, "lora_dgrad.g_t")
    for t, nm in ((a_qT, "a_qT"), (a_vT, "a_vT"), (out, "out")):
        _req16(t, "lora_dgrad." + nm, like=g_t)
    M, H = out.shape
    _need(g_t, M * 64, "lora_dgrad.g_t")
    _need(a_qT, H * 64, "lora_dgrad.a_qT")
    _need(a_vT, H * 64, "lora_dgrad.a_vT")
    p, seed, site = _drop(dropout)
    check(lib().tcavt_lora_dgrad(ptr(g_t), ptr(a_qT), ptr(a_vT), ptr(out), M, H, p, seed, site,
                                 (site + 1) if site_v is None else int(site_v), _DT[g_t.dtype], stream_ptr()), "tcavt_lora_dgrad")


def copy_batch(dsts, srcs):
    """dsts[i].copy_(srcs[i]) for up to 16 (device tensor, pinned host tensor) pairs of equal size, as ONE kernel launch on the
    current stream (tcavt_copy_batch: the copying lanes read the pinned memory over the host link; no copy-engine transfer)."""
    n = len(dsts)
    if n != len(srcs) or not 0 < n <= 16:
        raise capi.TcavtError("copy_batch: 1 .. 16 (dst, src) pairs")
    D, S, Bn = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)(), (ctypes.c_int64 * n)()
    for i, (d, s) in enumerate(zip(dsts, srcs)):
        nb = d.numel() * d.element_size()
        if s.numel() * s.element_size() != nb or d.dtype != s.dtype or not d.is_contiguous() or not s.is_contiguous():
            raise capi.TcavtError(f"copy_batch: pair {i}: contiguous tensors of one dtype and size required")
        if not (d.is_cuda or _ALLOW_CPU) or not (s.is_cuda or s.is_pinned() or _ALLOW_CPU):
            raise capi.TcavtError(f"copy_batch: pair {i}: dst on the GPU, src on the GPU or in pinned host memory")
        D[i], S[i], Bn[i] = d.data_ptr(), s.data_ptr(), nb
    check(lib().tcavt_copy_batch(D, S, Bn, n, stream_ptr()), "tcavt_copy_batch")


def sample_workspace(B, device):
    """Workspace of the two-stage token selection for B samples (tcavt_sample_workspace_bytes): uint8, zeroed once here; every
    call leaves its control words zero.  Calls that share it must be stream-ordered."""
    return torch.zeros(int(lib().tcavt_sample_workspace_bytes(int(B))), dtype=torch.uint8, device=device)


def _require(who, *tensors):
    """Every (tensor, dtype, entries, name) in turn: present, of that dtype, contiguous, of at least that many entries."""
    for t, dt, k, nm in tensors:
        if t is None:
            raise capi.TcavtError(f"{who}: {nm} is missing")
        _req(t, dt, f"{who}.{nm}")
        _need(t, k, f"{who}.{nm}")


def _sampler_guard(who, logits, workspace, n, step_n, out_n, history, hist_len, step, cur_tok, pos, finished, out_tokens, slots=None):
    """Host guard shared by the sampler wrappers: dtype, contiguity and minimal size of the logits, the workspace and the state
    -- ``n`` entries per state array, ``step_n`` step words, ``out_n`` output ids; slots = (max_new, out_row) in the per-slot forms."""
    if workspace is not None:
        _req(workspace, torch.uint8, f"{who}.workspace")
    _req(logits, torch.float32, f"{who}.logits")
    per_slot = () if slots is None else ((slots[0], torch.int32, n, "max_new"), (slots[1], torch.int64, n, "out_row"))
    _require(who, (history, torch.int64, n, "history"), (hist_len, torch.int32, n, "hist_len"), (step, torch.int32, step_n, "step"),
             *per_slot, (cur_tok, torch.int64, n, "cur_tok"), (pos, torch.int32, n, "pos"), (finished, torch.int32, n, "finished"),
             (out_tokens, torch.int64, out_n, "out_tokens"))


def _form(rows, state_rows, slot_of_row, *per_slot):
    """The form of a token selection on ``rows`` logits rows follows from its arguments, as in the C entries: slot_of_row -> the
    rows of a grouped admission on a state of ``state_rows`` slots; one of the ``per_slot`` arrays (out_row, max_new) -> decode
    slots; neither -> a batch.  -> (slots: a per-slot form, n: the state's rows, the number of step words)."""
    slots = slot_of_row is not None or any(t is not None for t in per_slot)
    n = state_rows if slot_of_row is not None else rows
    return slots, n, n if slots else 1


def _bracket_form(who, rows, state_rows, step, out_row, slot_of_row):
    """_form for a bracket around a token selection (logprob, constraint), which knows the per-slot forms by out_row alone:
    -> (slots, n, the _require entries of the three arrays the form is read from)."""
    if slot_of_row is not None and out_row is None:
        raise capi.TcavtError(f"{who}: out_row is missing (slot_of_row is given)")
    slots, n, step_n = _form(rows, state_rows, slot_of_row, out_row)
    per_slot = ((out_row, torch.int64, n, "out_row"),) if slots else ()
    per_row = ((slot_of_row, torch.int32, rows, "slot_of_row"),) if slot_of_row is not None else ()
    return slots, n, ((step, torch.int32, step_n, "step"), *per_slot, *per_row)


def _sample_args(logits, rows, n_state, history, hist_len, params, step, max_new, out_row, cur_tok, pos, finished, out_tokens,
                 advance_pos, workspace, stop, slot_of_row=None):
    """The tcavt_sample_args of a selection on the first ``rows`` logits rows and a state of ``n_state`` rows (the tensors are
    checked by the caller).  stop: a stopping.DeviceStopRules, a capi.StopRules struct or None."""
    a = capi.SampleArgs()
    a.logits, a.slot_of_row, a.history, a.hist_len = logits.data_ptr(), ptr(slot_of_row), history.data_ptr(), hist_len.data_ptr()
    a.params, a.step, a.max_new, a.out_row = ctypes.pointer(params), step.data_ptr(), ptr(max_new), ptr(out_row)
    a.cur_tok, a.pos, a.finished, a.out_tokens = cur_tok.data_ptr(), pos.data_ptr(), finished.data_ptr(), out_tokens.data_ptr()
    a.workspace, a.workspace_bytes = ptr(workspace), workspace.numel() if workspace is not None else 0
    if stop is not None:
        a.stop = ctypes.pointer(stop) if isinstance(stop, capi.StopRules) else stop.pointer()
    a.rows, a.V, a.n_state, a.hist_cap, a.out_cap = rows, logits.shape[1], n_state, history.shape[1], out_tokens.shape[1]
    a.advance_pos = int(advance_pos)
    return a


def sample_logits(logits, history, hist_len, params, step, cur_tok, pos, finished, out_tokens, advance_pos, workspace=None):
    """Logits processors + token selection (tcavt_sample_logits); every tensor is device state that the call advances.
    workspace (sample_workspace(B, device)): the two-stage form -- B x 16 workgroups instead of B; same tokens."""
    B, V = logits.shape
    _sampler_guard("sample_logits", logits, workspace, B, 1, B, history, hist_len, step, cur_tok, pos, finished, out_tokens)
    if history.shape[0] != B or out_tokens.shape[0] != B:
        raise capi.TcavtError("sample_logits: history / out_tokens need one row per sample")
    check(lib().tcavt_sample_logits(ptr(logits), B, V, ptr(history), history.shape[1], ptr(hist_len), ctypes.byref(params),
                                    ptr(step), ptr(cur_tok), ptr(pos), ptr(finished), ptr(out_tokens), out_tokens.shape[1],
                                    int(advance_pos), ptr(workspace), workspace.numel() if workspace is not None else 0,
                                    stream_ptr()), "tcavt_sample_logits")


def sample_logits_slots(logits, history, hist_len, params, step, max_new, out_row, cur_tok, pos, finished, out_tokens, advance_pos,
                        workspace=None):
    """sample_logits with per-slot bookkeeping (tcavt_sample_logits_slots): step / max_new int32 [S], out_row int64 [S] -- slot s
    chooses token step[s] of out_tokens[out_row[s]] (its Philox row too), ends on EOS or at its budget, and is inert once finished.
    The state tensors may be views that start at a slot (one-row logits of a request being admitted)."""
    S, V = logits.shape
    _sampler_guard("sample_logits_slots", logits, workspace, S, S, 1, history, hist_len, step, cur_tok, pos, finished, out_tokens,
                   slots=(max_new, out_row))
    if history.dim() != 2 or history.shape[0] != S or out_tokens.dim() != 2:
        raise capi.TcavtError("sample_logits_slots: history needs one row per slot, out_tokens one row per request")
    check(lib().tcavt_sample_logits_slots(ptr(logits), S, V, ptr(history), history.shape[1], ptr(hist_len), ctypes.byref(params),
                                          ptr(step), ptr(max_new), ptr(out_row), ptr(cur_tok), ptr(pos), ptr(finished),
                                          ptr(out_tokens), out_tokens.shape[1], int(advance_pos), ptr(workspace),
                                          workspace.numel() if workspace is not None else 0, stream_ptr()),
          "tcavt_sample_logits_slots")


def _bind_caches(a, who, src, dst, n_src, n_dst, src_lmax, kv_lmax, n_layers, nkv):
    """Into the args struct ``a`` (tcavt_slot_admit[_group]_args, tcavt_kv_fanout_args): the caches of the n_src-sample source and
    of the n_dst-sample destination -- both the 16-bit pair or both the four KV8 planes -- each checked first (``who`` in the errors)."""
    if len(src) != len(dst) or len(src) not in (2, 4):
        raise capi.TcavtError(f"{who}: src and dst are both (k, v) or both (k_codes, k_scales, v_codes, v_scales)")
    if len(src) == 2:
        for t, nm, lmax, n in ((src[0], "src_k", src_lmax, n_src), (src[1], "src_v", src_lmax, n_src), (dst[0], "dst_k", kv_lmax, n_dst),
                               (dst[1], "dst_v", kv_lmax, n_dst)):
            _req16(t, f"{who}.{nm}", like=src[0])
            _need(t, n_layers * n * lmax * nkv * 64, f"{who}.{nm}")
            capi.bind(a, **{nm: t})
        a.dtype16 = _DT[src[0].dtype]
    else:
        _kv8_planes(src, n_layers * n_src * nkv * src_lmax, f"{who}.src")
        _kv8_planes(dst, n_layers * n_dst * nkv * kv_lmax, f"{who}.dst")
        for side, planes in (("src", src), ("dst", dst)):
            for t, nm in zip(planes, ("k_codes", "k_scales", "v_codes", "v_scales")):
                capi.bind(a, **{f"{side}_{nm}": t})
        a.dtype16 = capi.F16  # (bytes are copied: the planes have no 16-bit type)


def _bind_admit(a, who, src, dst, n_src, src_lmax, kv_lmax, n_layers, S, nkv, history, hist_len, step, max_new, out_row, pos, finished,
                cur_tok):
    """Into the tcavt_slot_admit[_group]_args ``a``: the caches of the n_src-sample source and of the S-slot pool (_bind_caches) and
    the pool's eight slot-state arrays, each checked first (``who`` in the errors)."""
    _bind_caches(a, who, src, dst, n_src, S, src_lmax, kv_lmax, n_layers, nkv)
    for t, dt, nm in ((history, torch.int64, "history"), (hist_len, torch.int32, "hist_len"), (step, torch.int32, "step"),
                      (max_new, torch.int32, "max_new"), (out_row, torch.int64, "out_row"), (pos, torch.int32, "pos"),
                      (finished, torch.int32, "finished"), (cur_tok, torch.int64, "cur_tok")):
        _req(t, dt, f"{who}.{nm}")
        _need(t, S, f"{who}.{nm}")
        capi.bind(a, **{nm: t})
    if history.dim() != 2 or history.shape[0] != S:
        raise capi.TcavtError(f"{who}: history needs one row per slot")
    a.n_layers, a.S, a.src_lmax, a.kv_lmax, a.nkv, a.hist_cap = n_layers, S, src_lmax, kv_lmax, nkv, history.shape[1]


def slot_admit(src, dst, slot, rows, src_lmax, kv_lmax, n_layers, S, nkv, prompt_ids, kv_len, n_image, max_new_value, out_row_value,
               history, hist_len, step, max_new, out_row, pos, finished, cur_tok):
    """A freshly prefilled request moves into slot `slot` of an S-slot pool in one launch (tcavt_slot_admit).  src / dst: the
    one-sample cache and the pool's cache, both (k, v) 16-bit [n_layers, 1 | S, lmax, nkv * 64] or both the four KV8 planes
    (k_codes, k_scales, v_codes, v_scales) [n_layers, 1 | S, nkv, lmax, 64 | 2]; rows 0 .. rows - 1 are copied byte for byte.
    The slot's state: history row = prompt_ids, hist_len = *kv_len - n_image, pos = *kv_len, step = 0, finished = 0, max_new and
    out_row as given; cur_tok is left for the sampler."""
    a = capi.SlotAdmitArgs()
    _bind_admit(a, "slot_admit", src, dst, 1, src_lmax, kv_lmax, n_layers, S, nkv, history, hist_len, step, max_new, out_row, pos,
                finished, cur_tok)
    _req(prompt_ids, torch.int64, "slot_admit.prompt_ids")
    _req(kv_len, torch.int32, "slot_admit.kv_len")
    _need(kv_len, 1, "slot_admit.kv_len")
    a.prompt_ids, a.kv_len = prompt_ids.data_ptr(), kv_len.data_ptr()
    a.slot, a.rows, a.n_ids, a.n_image = int(slot), int(rows), prompt_ids.numel(), int(n_image)
    a.max_new_value, a.out_row_value = int(max_new_value), int(out_row_value)
    check(lib().tcavt_slot_admit(ctypes.byref(a), stream_ptr()), "tcavt_slot_admit")


def sample_logits_rows(logits, slot_of_row, history, hist_len, params, step, max_new, out_row, cur_tok, pos, finished, out_tokens,
                       advance_pos, workspace=None):
    """sample_logits_slots for the G logits rows of a grouped admission (tcavt_sample_logits_rows): logits [G, V]; slot_of_row int32
    [G] on the device; row g chooses the token of slot slot_of_row[g] of the S-slot state (history [S, cap] and the [S] arrays);
    a row whose entry is negative or >= S is skipped.  workspace: sample_workspace(G, device)."""
    G, V = logits.shape
    _req(slot_of_row, torch.int32, "sample_logits_rows.slot_of_row")
    _need(slot_of_row, G, "sample_logits_rows.slot_of_row")
    if history.dim() != 2 or out_tokens.dim() != 2:
        raise capi.TcavtError("sample_logits_rows: history needs one row per slot, out_tokens one row per request")
    S = history.shape[0]
    _sampler_guard("sample_logits_rows", logits, workspace, S, S, 1, history, hist_len, step, cur_tok, pos, finished, out_tokens,
                   slots=(max_new, out_row))
    check(lib().tcavt_sample_logits_rows(ptr(logits), G, V, ptr(slot_of_row), S, ptr(history), history.shape[1], ptr(hist_len),
                                         ctypes.byref(params), ptr(step), ptr(max_new), ptr(out_row), ptr(cur_tok), ptr(pos),
                                         ptr(finished), ptr(out_tokens), out_tokens.shape[1], int(advance_pos), ptr(workspace),
                                         workspace.numel() if workspace is not None else 0, stream_ptr()),
          "tcavt_sample_logits_rows")


class RequestTable:
    """Per-request sampler parameters (tcavt_request_params): ``params`` -- a sequence of capi.SampleParams, one per request -- and
    optionally one min_new_tokens per request, checked on the host by tcavt_request_params_check when built (TcavtError names the
    failing index and field; has_stop_bitmap: a stop set exists, so a positive minimum has something to ban without an EOS).
    ``to(device)`` uploads the tables, once, and makes ``flag``: device int32 [1], zeroed, that a row whose request index lies
    outside the table sets."""

    def __init__(self, params, min_new_tokens=None, has_stop_bitmap=False):
        n = self.n_req = len(params)
        if min_new_tokens is not None and len(min_new_tokens) != n:
            raise capi.TcavtError(f"RequestTable: {len(min_new_tokens)} min_new_tokens for {n} requests")
        self.host = (capi.SampleParams * max(n, 1))(*params)
        self.host_min = None if min_new_tokens is None else (ctypes.c_int32 * max(n, 1))(*[int(m) for m in min_new_tokens])
        # (host only: the library itself, also where ops runs against a stand-in)
        rc = capi.lib().tcavt_request_params_check(self.host, self.host_min, n, int(bool(has_stop_bitmap)))
        if rc != 0:
            raise capi.TcavtError(f"tcavt_request_params_check failed (code {rc}): {capi.lib().tcavt_last_error().decode()}")
        self.table = self.min_new = self.flag = self._struct = None

    def to(self, device):
        self.table = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).to(device)
        self.min_new = None if self.host_min is None else torch.tensor(list(self.host_min), dtype=torch.int32).to(device)
        self.flag = torch.zeros(1, dtype=torch.int32, device=device)
        self._struct = None
        return self

    def pointer(self):
        if self._struct is None:
            r = capi.RequestParams()
            r.table = ctypes.cast(self.table.data_ptr(), ctypes.POINTER(capi.SampleParams))
            capi.bind(r, min_new_tokens=self.min_new, bad_index_flag=self.flag)
            r.n_req = self.n_req
            self._struct = r
        return ctypes.pointer(self._struct)


def sample_tokens(logits, history, hist_len, params, step, cur_tok, pos, finished, out_tokens, advance_pos, workspace=None,
                  max_new=None, out_row=None, slot_of_row=None, stop=None, per_request=None):
    """The three token-selection entries in one, with optional ending rules (tcavt_sample_tokens).  The form follows from the
    arguments as in the C entry: slot_of_row -> sample_logits_rows, max_new / out_row -> sample_logits_slots, neither ->
    sample_logits.  stop: a stopping.DeviceStopRules (or a capi.StopRules struct), or None -- then, and with nothing set in it,
    the launches are those of the corresponding existing entry.  per_request: a RequestTable (or a capi.RequestParams struct) ->
    tcavt_sample_tokens_per_request: every row takes its parameters from the table at its request index (the row in the batch
    form, out_row[slot] otherwise); ``params`` still carries the call's pad_token_id."""
    rows, _ = logits.shape
    if history.dim() != 2 or out_tokens.dim() != 2:
        raise capi.TcavtError("sample_tokens: history needs one row per sample / slot, out_tokens one row per sample / request")
    slots, n, step_n = _form(rows, history.shape[0], slot_of_row, max_new, out_row)
    if history.shape[0] != n or (not slots and out_tokens.shape[0] != rows):
        raise capi.TcavtError("sample_tokens: history / out_tokens need one row per sample")
    if slot_of_row is not None:
        _req(slot_of_row, torch.int32, "sample_tokens.slot_of_row")
        _need(slot_of_row, rows, "sample_tokens.slot_of_row")
    _sampler_guard("sample_tokens", logits, workspace, n, step_n, 1, history, hist_len, step, cur_tok, pos, finished, out_tokens,
                   slots=(max_new, out_row) if slots else None)
    a = _sample_args(logits, rows, n, history, hist_len, params, step, max_new, out_row, cur_tok, pos, finished, out_tokens,
                     advance_pos, workspace, stop, slot_of_row)
    if per_request is not None:
        if not isinstance(per_request, capi.RequestParams):
            _req(per_request.table, torch.uint8, "sample_tokens.per_request.table")
            _req(per_request.min_new, torch.int32, "sample_tokens.per_request.min_new")
            _need(per_request.min_new, per_request.n_req, "sample_tokens.per_request.min_new")
            _need(per_request.table, per_request.n_req * ctypes.sizeof(capi.SampleParams), "sample_tokens.per_request.table")
            if not slots and per_request.n_req < rows:
                raise capi.TcavtError(f"sample_tokens: per_request has {per_request.n_req} entries for {rows} rows")
        req = ctypes.pointer(per_request) if isinstance(per_request, capi.RequestParams) else per_request.pointer()
        check(lib().tcavt_sample_tokens_per_request(ctypes.byref(a), req, stream_ptr()), "tcavt_sample_tokens_per_request")
        return
    check(lib().tcavt_sample_tokens(ctypes.byref(a), stream_ptr()), "tcavt_sample_tokens")


def logprob_workspace_bytes(rows, hist_cap):
    """Bytes of the workspace of logprob_begin / logprob_finish for ``rows`` logits rows and histories of ``hist_cap`` ids."""
    return int(capi.lib().tcavt_logprob_workspace_bytes(int(rows), int(hist_cap)))


def logprob_args(logits, history, hist_len, step, finished, out_tokens, token_logprobs, sum_logprob, n_scored, workspace,
                 out_row=None, slot_of_row=None):
    """The tcavt_logprob_args of one bracket around a token selection on the same logits and state (the form follows from
    slot_of_row / out_row as in sample_tokens), each tensor checked first.  token_logprobs fp32 like out_tokens; sum_logprob fp32
    and n_scored int32, one entry per row of out_tokens; workspace uint8 of logprob_workspace_bytes(rows, history.shape[1])."""
    who = "logprob"
    rows, V = logits.shape
    if history.dim() != 2 or out_tokens.dim() != 2:
        raise capi.TcavtError("logprob: history needs one row per sample / slot, out_tokens one row per sample / request")
    slots, n, form = _bracket_form(who, rows, history.shape[0], step, out_row, slot_of_row)
    if history.shape[0] != n or (not slots and out_tokens.shape[0] != rows):
        raise capi.TcavtError("logprob: history / out_tokens need one row per sample")
    if token_logprobs.shape != out_tokens.shape:
        raise capi.TcavtError("logprob: token_logprobs must have the shape of out_tokens")
    _req(logits, torch.float32, f"{who}.logits")
    n_out = out_tokens.shape[0]
    _require(who, (history, torch.int64, n, "history"), (hist_len, torch.int32, n, "hist_len"), *form,
             (finished, torch.int32, n, "finished"), (out_tokens, torch.int64, 1, "out_tokens"),
             (token_logprobs, torch.float32, 1, "token_logprobs"), (sum_logprob, torch.float32, n_out, "sum_logprob"),
             (n_scored, torch.int32, n_out, "n_scored"),
             (workspace, torch.uint8, logprob_workspace_bytes(rows, history.shape[1]), "workspace"))
    a = capi.LogprobArgs()
    a.logits, a.slot_of_row, a.history, a.hist_len = logits.data_ptr(), ptr(slot_of_row), history.data_ptr(), hist_len.data_ptr()
    a.step, a.out_row, a.finished, a.out_tokens = step.data_ptr(), ptr(out_row), finished.data_ptr(), out_tokens.data_ptr()
    a.token_logprobs, a.sum_logprob, a.n_scored = token_logprobs.data_ptr(), sum_logprob.data_ptr(), n_scored.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
    a.rows, a.V, a.n_state, a.hist_cap, a.out_cap = rows, V, n, history.shape[1], out_tokens.shape[1]
    return a


def logprob_begin(args):
    """Before the token selection: the raw row's (max, sum exp) partials and the snapshot (tcavt_logprob_begin)."""
    check(lib().tcavt_logprob_begin(ctypes.byref(args), stream_ptr()), "tcavt_logprob_begin")


def logprob_finish(args):
    """After the token selection: log_softmax(raw)[token] of every row that was live (tcavt_logprob_finish)."""
    check(lib().tcavt_logprob_finish(ctypes.byref(args), stream_ptr()), "tcavt_logprob_finish")


TOP_LOGPROBS_MAX = 20  # k of tcavt_logprob_topk


def logprob_topk_workspace_bytes(rows, k):
    """Bytes of the workspace of logprob_topk for ``rows`` logits rows and lists of ``k`` entries."""
    return int(capi.lib().tcavt_logprob_topk_workspace_bytes(int(rows), int(k)))


def logprob_topk_args(lp_args, out_tokens, top_ids, top_logprobs, workspace):
    """The tcavt_logprob_topk_args of one launch inside the bracket ``lp_args`` (a capi.LogprobArgs from logprob_args, made with
    the same ``out_tokens``), each tensor checked first.  top_ids int32 and top_logprobs fp32 [*out_tokens.shape, k], k = their
    last dimension; workspace uint8 of logprob_topk_workspace_bytes(rows, k), its own."""
    who = "logprob_topk"
    if not isinstance(lp_args, capi.LogprobArgs):
        raise capi.TcavtError(f"{who}: lp_args must be the capi.LogprobArgs of the bracket")
    if top_ids is None or top_logprobs is None or workspace is None:
        raise capi.TcavtError(f"{who}: top_ids, top_logprobs and workspace are required")
    if out_tokens.dim() != 2 or out_tokens.data_ptr() != lp_args.out_tokens or out_tokens.shape[1] != lp_args.out_cap:
        raise capi.TcavtError(f"{who}: out_tokens is not the one of the bracket")
    if top_ids.dim() != 3 or tuple(top_ids.shape[:2]) != tuple(out_tokens.shape) or top_logprobs.shape != top_ids.shape:
        raise capi.TcavtError(f"{who}: top_ids and top_logprobs must be [*out_tokens.shape, k], got {tuple(top_ids.shape)} and "
                              f"{tuple(top_logprobs.shape)} for out_tokens {tuple(out_tokens.shape)}")
    k = int(top_ids.shape[2])
    if not 1 <= k <= TOP_LOGPROBS_MAX or k > lp_args.V:
        raise capi.TcavtError(f"{who}: k = {k} must be in [1, {TOP_LOGPROBS_MAX}] and <= V = {lp_args.V}")
    for t, dt, n, nm in ((top_ids, torch.int32, out_tokens.numel() * k, "top_ids"),
                         (top_logprobs, torch.float32, out_tokens.numel() * k, "top_logprobs"),
                         (workspace, torch.uint8, logprob_topk_workspace_bytes(lp_args.rows, k), "workspace")):
        _req(t, dt, f"{who}.{nm}")
        _need(t, n, f"{who}.{nm}")
    a = capi.LogprobTopkArgs()
    a.lp = ctypes.pointer(lp_args)  # (the struct keeps the bracket's alive)
    a.top_ids, a.top_logprobs = top_ids.data_ptr(), top_logprobs.data_ptr()
    a.workspace, a.workspace_bytes, a.k = workspace.data_ptr(), workspace.numel(), k
    return a


def logprob_topk(args):
    """Between logprob_begin and the first writer of the logits: the raw row's k most likely tokens (tcavt_logprob_topk)."""
    check(lib().tcavt_logprob_topk(ctypes.byref(args), stream_ptr()), "tcavt_logprob_topk")


class ConstraintTable:
    """The device side of a constraint.TokenConstraint (tcavt_constraint_table): token_class int32 [V] and trans int32 [n_states,
    n_classes] uploaded, bitmap int32 [n_states, ceil(V / 32)] (the uint32 words) and count int32 [n_states] made by ``build()``
    (tcavt_constraint_build), once per call of a generate entry."""

    def __init__(self, token_class, trans, device):
        for t, dim, nm in ((token_class, 1, "token_class"), (trans, 2, "trans")):
            if t.dtype != torch.int32 or t.dim() != dim:
                raise capi.TcavtError(f"constraint table: {nm} must be an int32 tensor with {dim} dimension(s)")
        self.V, (self.n_states, self.n_classes) = token_class.numel(), trans.shape
        self.token_class, self.trans = token_class.contiguous().to(device), trans.contiguous().to(device)
        self.bitmap = torch.empty(self.n_states, (self.V + 31) // 32, dtype=torch.int32, device=device)
        self.count = torch.empty(self.n_states, dtype=torch.int32, device=device)
        t = self.struct = capi.ConstraintTable()
        capi.bind(t, token_class=self.token_class, trans=self.trans, bitmap=self.bitmap, count=self.count)
        t.V, t.n_states, t.n_classes = self.V, self.n_states, self.n_classes

    def build(self):
        check(lib().tcavt_constraint_build(ctypes.byref(self.struct), stream_ptr()), "tcavt_constraint_build")
        return self


def constraint_workspace_bytes(rows):
    """Bytes of the workspace of constraint_mask / constraint_advance for ``rows`` logits rows."""
    return int(capi.lib().tcavt_constraint_workspace_bytes(int(rows)))


def constraint_args(table, logits, step, finished, cur_tok, state, start, workspace, out_row=None, slot_of_row=None,
                    request_state=None, flag=None):
    """The tcavt_constraint_args of one bracket around a token selection on the same logits and state (the form follows from
    slot_of_row / out_row as in sample_tokens), each tensor checked first.  table: a built ConstraintTable; state int32, one word
    per sample / slot; start int32 [n_req], the start state of every request; request_state int32 [n_req] and flag int32 [1]
    optional; workspace uint8 of constraint_workspace_bytes(rows)."""
    who = "constraint"
    rows, V = logits.shape
    if V != table.V:
        raise capi.TcavtError(f"constraint: the table is over {table.V} token ids, the logits have {V}")
    slots, n, form = _bracket_form(who, rows, 0 if state is None else state.numel(), step, out_row, slot_of_row)
    n_req = start.numel()
    if not slots and n_req < rows:
        raise capi.TcavtError(f"constraint: start has {n_req} entries for {rows} rows")
    _req(logits, torch.float32, f"{who}.logits")
    optional = tuple((t, torch.int32, k, nm) for t, k, nm in ((request_state, n_req, "request_state"), (flag, 1, "flag")) if t is not None)
    _require(who, *form, (finished, torch.int32, n, "finished"), (cur_tok, torch.int64, n, "cur_tok"), (state, torch.int32, n, "state"),
             (start, torch.int32, 1, "start"), *optional, (workspace, torch.uint8, constraint_workspace_bytes(rows), "workspace"))
    a = capi.ConstraintArgs()
    a.table = ctypes.pointer(table.struct)
    capi.bind(a, logits=logits, slot_of_row=slot_of_row, step=step, out_row=out_row, finished=finished, cur_tok=cur_tok, state=state,
              start=start, request_state=request_state, flag=flag, workspace=workspace)
    a.workspace_bytes, a.rows, a.n_state, a.n_req = workspace.numel(), rows, n, n_req
    return a


def constraint_mask(args):
    """Before the token selection: -inf over the tokens the row's state does not allow (tcavt_constraint_mask)."""
    check(lib().tcavt_constraint_mask(ctypes.byref(args), stream_ptr()), "tcavt_constraint_mask")


def constraint_advance(args):
    """After the token selection: the state of every row that was live follows the chosen token (tcavt_constraint_advance)."""
    check(lib().tcavt_constraint_advance(ctypes.byref(args), stream_ptr()), "tcavt_constraint_advance")


BEAMS_MAX = 16  # beams per prompt of tcavt_beam_select / tcavt_beam_reorder


def beam_workspace_bytes(R):
    """Bytes of the workspace of beam_select for R = B * n decode rows."""
    return int(capi.lib().tcavt_beam_workspace_bytes(int(R)))


def beam_args(logits, n, N, history, hist_len, run_score, live, fin_tokens, fin_score, fin_flag, fin_len, unsat, done, cur_tok, pos,
              finished, step, prefix_len, len_pow, parent, plan, workspace, eos_token_id, pad_token_id, repetition_penalty,
              no_repeat_ngram_size, early_stopping, trace=None):
    """The tcavt_beam_args of a beam search on R = B * n rows (logits fp32 [R, V]; the per-row, per-prompt and finished-store
    tensors as include/tcavt.h lists them), each tensor checked first.  The struct names fixed device arrays: one serves every
    step of a call, captured or not."""
    who = "beam_select"
    R, V = logits.shape
    n, N = int(n), int(N)
    if n < 1 or R % n != 0:
        raise capi.TcavtError(f"{who}: {R} logits rows do not make prompts of n = {n} beams")
    B = R // n
    if history.dim() != 2 or history.shape[0] != R:
        raise capi.TcavtError(f"{who}: history needs one row per decode row")
    _require(who, (logits, torch.float32, R * V, "logits"), (history, torch.int64, R, "history"), (hist_len, torch.int32, R, "hist_len"),
             (run_score, torch.float32, R, "run_score"), (live, torch.int32, R, "live"),
             (fin_tokens, torch.int64, R * N, "fin_tokens"), (fin_score, torch.float32, R, "fin_score"),
             (fin_flag, torch.int32, R, "fin_flag"), (fin_len, torch.int32, R, "fin_len"), (unsat, torch.int32, B, "unsat"),
             (done, torch.int32, B, "done"), (cur_tok, torch.int64, R, "cur_tok"), (pos, torch.int32, R, "pos"),
             (finished, torch.int32, R, "finished"), (step, torch.int32, B, "step"), (prefix_len, torch.int32, B, "prefix_len"),
             (len_pow, torch.float32, N, "len_pow"), (parent, torch.int32, R, "parent"), (plan, torch.int32, 4 * B, "plan"),
             (workspace, torch.uint8, beam_workspace_bytes(R), "workspace"))
    _req(trace, torch.int32, f"{who}.trace")
    _need(trace, N * B * 2 * n * 3, f"{who}.trace")
    a = capi.BeamArgs()
    capi.bind(a, logits=logits, history=history, hist_len=hist_len, run_score=run_score, live=live, fin_tokens=fin_tokens,
              fin_score=fin_score, fin_flag=fin_flag, fin_len=fin_len, unsat=unsat, done=done, cur_tok=cur_tok, pos=pos,
              finished=finished, step=step, prefix_len=prefix_len, len_pow=len_pow, parent=parent, plan=plan, trace=trace,
              workspace=workspace)
    a.workspace_bytes = workspace.numel()
    a.eos_token_id, a.pad_token_id = -1 if eos_token_id is None else int(eos_token_id), int(pad_token_id)
    a.repetition_penalty, a.no_repeat_ngram_size, a.early_stopping = float(repetition_penalty), int(no_repeat_ngram_size), int(bool(early_stopping))
    a.R, a.n, a.V, a.N, a.hist_cap = R, n, V, N, history.shape[1]
    return a


def beam_select(args):
    """One step's selection of a beam search (tcavt_beam_select): candidates, new beams, finished store, done flags, the plan."""
    check(lib().tcavt_beam_select(ctypes.byref(args), stream_ptr()), "tcavt_beam_select")


def beam_reorder_args(n, parent, plan, cur_tok, history, hist_len, pos, step, suffix_k, suffix_v, n_layers, nkv):
    """The tcavt_beam_reorder_args of the same search: suffix_k / suffix_v 16-bit [n_layers, R, suffix_lmax, nkv * 64]."""
    who = "beam_reorder"
    R, n = parent.numel(), int(n)
    if n < 1 or R % n != 0:
        raise capi.TcavtError(f"{who}: {R} rows do not make prompts of n = {n} beams")
    B = R // n
    if history.dim() != 2 or history.shape[0] != R or suffix_k.dim() != 4 or suffix_k.shape != suffix_v.shape:
        raise capi.TcavtError(f"{who}: history needs one row per decode row, suffix_k / suffix_v [n_layers, R, suffix_lmax, nkv * 64]")
    if tuple(suffix_k.shape[:2]) != (n_layers, R) or suffix_k.shape[3] != nkv * 64:
        raise capi.TcavtError(f"{who}: suffix caches of shape {tuple(suffix_k.shape)} for n_layers = {n_layers}, R = {R}, nkv = {nkv}")
    for t, dt, k, nm in ((parent, torch.int32, R, "parent"), (plan, torch.int32, 4 * B, "plan"), (cur_tok, torch.int64, R, "cur_tok"),
                         (history, torch.int64, R, "history"), (hist_len, torch.int32, R, "hist_len"), (pos, torch.int32, R, "pos"),
                         (step, torch.int32, B, "step")):
        _req(t, dt, f"{who}.{nm}")
        _need(t, k, f"{who}.{nm}")
    _req16(suffix_k, f"{who}.suffix_k")
    _req16(suffix_v, f"{who}.suffix_v", like=suffix_k)
    a = capi.BeamReorderArgs()
    capi.bind(a, parent=parent, plan=plan, cur_tok=cur_tok, history=history, hist_len=hist_len, pos=pos, step=step,
              suffix_k=suffix_k, suffix_v=suffix_v)
    a.R, a.n, a.hist_cap, a.n_layers, a.nkv, a.suffix_lmax = R, n, history.shape[1], int(n_layers), int(nkv), suffix_k.shape[2]
    return a


def beam_reorder(args):
    """Histories and suffix caches follow the parents of the last beam_select, in place (tcavt_beam_reorder)."""
    check(lib().tcavt_beam_reorder(ctypes.byref(args), stream_ptr()), "tcavt_beam_reorder")


def slot_admit_group(src, dst, slot, rows, src_lmax, kv_lmax, n_layers, S, nkv, prompt_ids, kv_len, n_image, max_new_value,
                     out_row_value, bad_slot_flag, history, hist_len, step, max_new, out_row, pos, finished, cur_tok):
    """The G samples of a grouped prefill move into their slots of an S-slot pool in one launch (tcavt_slot_admit_group).  src: the
    G-sample cache, dst: the pool's cache, both (k, v) 16-bit [n_layers, G | S, lmax, nkv * 64] or both the four KV8 planes
    [n_layers, G | S, nkv, lmax, 64 | 2].  Per row, on the device: slot int32 [G] (< 0: a pad row; >= S: nothing written,
    bad_slot_flag int32 [1] set; the slots of a group are distinct), kv_len int32 [G], max_new_value int32 [G], out_row_value int64
    [G], prompt_ids int64 [G, n_ids].  State of an admitted slot as slot_admit."""
    a = capi.SlotAdmitGroupArgs()
    _req(slot, torch.int32, "slot_admit_group.slot")
    G = slot.numel()
    if G < 1:
        raise capi.TcavtError("slot_admit_group: slot needs one entry per row of the group")
    _bind_admit(a, "slot_admit_group", src, dst, G, src_lmax, kv_lmax, n_layers, S, nkv, history, hist_len, step, max_new, out_row,
                pos, finished, cur_tok)
    if prompt_ids.dim() != 2 or prompt_ids.shape[0] != G:
        raise capi.TcavtError("slot_admit_group: prompt_ids needs one row per row of the group")
    for t, dt, n, nm in ((kv_len, torch.int32, G, "kv_len"), (max_new_value, torch.int32, G, "max_new_value"),
                         (out_row_value, torch.int64, G, "out_row_value"), (prompt_ids, torch.int64, G, "prompt_ids"),
                         (bad_slot_flag, torch.int32, 1, "bad_slot_flag")):
        _req(t, dt, "slot_admit_group." + nm)
        _need(t, n, "slot_admit_group." + nm)
        capi.bind(a, **{nm: t})
    a.slot, a.G, a.rows, a.n_ids, a.n_image = slot.data_ptr(), G, int(rows), prompt_ids.shape[1], int(n_image)
    check(lib().tcavt_slot_admit_group(ctypes.byref(a), stream_ptr()), "tcavt_slot_admit_group")


def _bind_fanout(a, who, n, prompt_ids, kv_len, n_image, logits_src, logits_dst, history, hist_len, pos, finished, caches=None):
    """Into the tcavt_kv_fanout_args / tcavt_state_fanout_args ``a``: B prompts become B * n decode rows -- the shapes, then the caches
    if there are any (``caches``: _bind_caches' arguments from src_lmax on), then the eight state tensors, each checked first
    (``who`` in the errors)."""
    if prompt_ids.dim() != 2 or logits_src.dim() != 2 or logits_dst.dim() != 2 or history.dim() != 2:
        raise capi.TcavtError(f"{who}: prompt_ids, logits_src, logits_dst and history are 2-D, one row per prompt / per decode row")
    B, n = prompt_ids.shape[0], int(n)
    if B < 1 or n < 1:
        raise capi.TcavtError(f"{who}: B = {B} and n = {n} must be >= 1")
    R, V = B * n, logits_src.shape[1]
    if logits_src.shape[0] != B or tuple(logits_dst.shape) != (R, V) or history.shape[0] != R:
        raise capi.TcavtError(f"{who}: logits_src needs B = {B} rows, logits_dst [{R}, {V}] and history {R} rows")
    if caches is not None:
        src, dst, *shape = caches
        _bind_caches(a, who, src, dst, B, R, *shape)
    for t, dt, k, nm in ((prompt_ids, torch.int64, B, "prompt_ids"), (kv_len, torch.int32, B, "kv_len"),
                         (logits_src, torch.float32, B * V, "logits_src"), (logits_dst, torch.float32, R * V, "logits_dst"),
                         (history, torch.int64, R, "history"), (hist_len, torch.int32, R, "hist_len"), (pos, torch.int32, R, "pos"),
                         (finished, torch.int32, R, "finished")):
        _req(t, dt, f"{who}.{nm}")
        _need(t, k, f"{who}.{nm}")
        capi.bind(a, **{nm: t})
    a.B, a.n, a.n_ids, a.hist_cap, a.n_image, a.V = B, n, prompt_ids.shape[1], history.shape[1], int(n_image), V


def kv_fanout(src, dst, n, rows, src_lmax, kv_lmax, n_layers, nkv, prompt_ids, kv_len, n_image, logits_src, logits_dst, history,
              hist_len, pos, finished):
    """A B-sample prefill becomes the state of a decode batch of B * n rows in one launch (tcavt_kv_fanout): row b * n + j is
    continuation j of prompt b.  src: the B-sample cache, dst: the cache of B * n samples, both (k, v) 16-bit [n_layers, B | B * n,
    lmax, nkv * 64] or both the four KV8 planes [n_layers, B | B * n, nkv, lmax, 64 | 2]; rows 0 .. rows - 1 are copied byte for
    byte, each piece of the source read once.  prompt_ids int64 [B, n_ids], kv_len int32 [B], logits_src fp32 [B, V] -> logits_dst
    [B * n, V], history int64 [B * n, cap] (its first n_ids columns), hist_len = kv_len - n_image, pos = kv_len, finished = 0."""
    a = capi.KvFanoutArgs()
    _bind_fanout(a, "kv_fanout", n, prompt_ids, kv_len, n_image, logits_src, logits_dst, history, hist_len, pos, finished,
                 caches=(src, dst, src_lmax, kv_lmax, n_layers, nkv))
    a.n_layers, a.rows, a.src_lmax, a.kv_lmax, a.nkv = n_layers, int(rows), src_lmax, kv_lmax, nkv
    check(lib().tcavt_kv_fanout(ctypes.byref(a), stream_ptr()), "tcavt_kv_fanout")


def state_fanout(n, prompt_ids, kv_len, n_image, logits_src, logits_dst, history, hist_len, pos, finished):
    """kv_fanout without a cache to copy (tcavt_state_fanout), for decode rows that read their prompt's cache in place: prompt_ids
    int64 [B, n_ids], kv_len int32 [B], logits_src fp32 [B, V] -> logits_dst [B * n, V], history int64 [B * n, cap] (its first n_ids
    columns), hist_len = kv_len - n_image, pos = kv_len, finished = 0 for row b * n + j."""
    a = capi.StateFanoutArgs()
    _bind_fanout(a, "state_fanout", n, prompt_ids, kv_len, n_image, logits_src, logits_dst, history, hist_len, pos, finished)
    check(lib().tcavt_state_fanout(ctypes.byref(a), stream_ptr()), "tcavt_state_fanout")


def gather_last(src16, kv_len, out16, B, L, H):
    _req16(src16, "gather_last.src16")
    _req16(out16, "gather_last.out16", like=src16)
    _req(kv_len, torch.int32, "gather_last.kv_len")
    _need(src16, B * L * H, "gather_last.src16")
    _need(out16, B * H, "gather_last.out16")
    _need(kv_len, B, "gather_last.kv_len")
    check(lib().tcavt_gather_last(ptr(src16), ptr(kv_len), ptr(out16), B, L, H, stream_ptr()), "tcavt_gather_last")


def attn_decode(qkv, k_cache, v_cache, pos, out, B, nq, nkv, kv_lmax, scale, out_layout=0):
    """The decode step's attention over ONE layer's cache [B, kv_lmax, nkv * 64] (tcavt_attn_decode): appends the qkv row's
    k | v at pos[b] and attends keys 0 .. pos[b].  out_layout 1 / 2: out in fragment-major order (16 / 32 or 8 whole rows)."""
    _req16(qkv, "attn_decode.qkv")
    for t, nm in ((k_cache, "k_cache"), (v_cache, "v_cache"), (out, "out")):
        _req16(t, "attn_decode." + nm, like=qkv)
    _req(pos, torch.int32, "attn_decode.pos")
    _need(qkv, B * (nq + 2 * nkv) * 64, "attn_decode.qkv")
    _need(k_cache, B * kv_lmax * nkv * 64, "attn_decode.k_cache")
    _need(v_cache, B * kv_lmax * nkv * 64, "attn_decode.v_cache")
    _need(pos, B, "attn_decode.pos")
    rows = B if out_layout == 0 else 8 if out_layout == 2 else 16 * ((B + 15) // 16)
    _need(out, rows * nq * 64, "attn_decode.out")
    check(lib().tcavt_attn_decode(ptr(qkv), ptr(k_cache), ptr(v_cache), ptr(pos), ptr(out), B, nq, nkv, kv_lmax, scale,
                                  _DT[qkv.dtype], int(out_layout), stream_ptr()), "tcavt_attn_decode")


def attn_decode_shared(qkv, prefix_k, prefix_v, prefix_len, suffix_k, suffix_v, pos, out, B, n, nq, nkv, prefix_lmax, suffix_lmax,
                       scale, out_layout=0):
    """attn_decode for the B * n rows of n continuations per prompt on ONE layer (tcavt_attn_decode_shared): the prompts' cache
    prefix_k / prefix_v [B, prefix_lmax, nkv * 64] (rows < prefix_len[b]) is read in place and never written, each row owns
    suffix_k / suffix_v [B * n, suffix_lmax, nkv * 64]; the qkv row's k | v go to suffix row pos[r] - prefix_len[r // n]."""
    who = "attn_decode_shared"
    R = B * n
    _req16(qkv, f"{who}.qkv")
    for t, nm in ((prefix_k, "prefix_k"), (prefix_v, "prefix_v"), (suffix_k, "suffix_k"), (suffix_v, "suffix_v"), (out, "out")):
        _req16(t, f"{who}.{nm}", like=qkv)
    _req(pos, torch.int32, f"{who}.pos")
    _req(prefix_len, torch.int32, f"{who}.prefix_len")
    _need(qkv, R * (nq + 2 * nkv) * 64, f"{who}.qkv")
    _need(prefix_k, B * prefix_lmax * nkv * 64, f"{who}.prefix_k")
    _need(prefix_v, B * prefix_lmax * nkv * 64, f"{who}.prefix_v")
    _need(suffix_k, R * suffix_lmax * nkv * 64, f"{who}.suffix_k")
    _need(suffix_v, R * suffix_lmax * nkv * 64, f"{who}.suffix_v")
    _need(prefix_len, B, f"{who}.prefix_len")
    _need(pos, R, f"{who}.pos")
    rows = R if out_layout == 0 else 8 if out_layout == 2 else 16 * ((R + 15) // 16)
    _need(out, rows * nq * 64, f"{who}.out")
    check(lib().tcavt_attn_decode_shared(ptr(qkv), ptr(prefix_k), ptr(prefix_v), ptr(prefix_len), ptr(suffix_k), ptr(suffix_v), ptr(pos),
                                         ptr(out), B, n, nq, nkv, prefix_lmax, suffix_lmax, scale, _DT[qkv.dtype], int(out_layout),
                                         stream_ptr()), "tcavt_attn_decode_shared")


def _kv8_planes(planes, rows, what):
    kcod, ksc, vcod, vsc = planes
    for t, nm, per in ((kcod, "k_codes", 64), (ksc, "k_scales", 2), (vcod, "v_codes", 64), (vsc, "v_scales", 2)):
        _req(t, torch.uint8, f"{what}.{nm}")
        _need(t, rows * per, f"{what}.{nm}")


def kv_store8(qkv, B, L, kv_lmax, nq, nkv, k_codes, k_scales, v_codes, v_scales):
    """Prefill store of ONE layer into the FP8 cache (tcavt_kv_store8): rows (b, l < L) of the rotated k | v columns of qkv
    [B * L, (nq + 2 nkv) * 64] -> positions l of the head-major planes, codes uint8 [B, nkv, kv_lmax, 64] and scale bytes uint8
    [B, nkv, kv_lmax, 2]; byte for byte quant.kv8_quantize."""
    _req16(qkv, "kv_store8.qkv")
    _need(qkv, B * L * (nq + 2 * nkv) * 64, "kv_store8.qkv")
    _kv8_planes((k_codes, k_scales, v_codes, v_scales), B * nkv * kv_lmax, "kv_store8")
    check(lib().tcavt_kv_store8(ptr(qkv), B, L, kv_lmax, nq, nkv, _DT[qkv.dtype], ptr(k_codes), ptr(k_scales), ptr(v_codes),
                                ptr(v_scales), stream_ptr()), "tcavt_kv_store8")


def attn_decode8(qkv, k_codes, k_scales, v_codes, v_scales, pos, out, B, nq, nkv, kv_lmax, scale, out_layout=0):
    """attn_decode over ONE layer's FP8 cache (tcavt_attn_decode8; planes as for kv_store8): appends the qkv row's k | v at
    pos[b], quantised, and attends the cached keys 0 .. pos[b] - 1 as code * 2^k plus the new key / value at 16-bit precision."""
    _req16(qkv, "attn_decode8.qkv")
    _req16(out, "attn_decode8.out", like=qkv)
    _req(pos, torch.int32, "attn_decode8.pos")
    _need(qkv, B * (nq + 2 * nkv) * 64, "attn_decode8.qkv")
    _kv8_planes((k_codes, k_scales, v_codes, v_scales), B * nkv * kv_lmax, "attn_decode8")
    _need(pos, B, "attn_decode8.pos")
    rows = B if out_layout == 0 else 8 if out_layout == 2 else 16 * ((B + 15) // 16)
    _need(out, rows * nq * 64, "attn_decode8.out")
    check(lib().tcavt_attn_decode8(ptr(qkv), ptr(k_codes), ptr(k_scales), ptr(v_codes), ptr(v_scales), ptr(pos), ptr(out), B, nq, nkv,
                                   kv_lmax, scale, _DT[qkv.dtype], int(out_layout), stream_ptr()), "tcavt_attn_decode8")


def llama_decode_step(args):
    """args: capi.DecodeArgs filled by generation.generate_batch (which owns and sizes every buffer)."""
    check(lib().tcavt_llama_decode_step(ctypes.byref(args), stream_ptr()), "tcavt_llama_decode_step")


def llama_decode_step_shared(args, prefix):
    """llama_decode_step for n continuations per prompt on the prompts' cache in place (tcavt_llama_decode_step_shared).  prefix:
    capi.KvPrefix; args.k_cache / v_cache are the suffix caches and args.kv_lmax counts their rows."""
    check(lib().tcavt_llama_decode_step_shared(ctypes.byref(args), ctypes.byref(prefix), stream_ptr()), "tcavt_llama_decode_step_shared")


def llama_decode_step_multi(args, T):
    """llama_decode_step for args.B = S * T rows, T consecutive positions of each of S sequences on one cache per sequence
    (tcavt_llama_decode_step_multi).  args.cur_tok / pos are the row arrays ngram_draft writes; args.k_cache / v_cache hold S
    sequences per layer."""
    check(lib().tcavt_llama_decode_step_multi(ctypes.byref(args), int(T), stream_ptr()), "tcavt_llama_decode_step_multi")


def attn_decode_multi(qkv, k_cache, v_cache, pos_rows, out, S, T, nq, nkv, kv_lmax, scale, out_layout=0):
    """attn_decode for T consecutive positions of each of S sequences on ONE layer's cache [S, kv_lmax, nkv * 64]
    (tcavt_attn_decode_multi): row r = s * T + j of qkv attends cache rows < base = pos_rows[s * T] and the new keys of rows
    s * T .. r, taken from qkv; cache rows base .. base + T - 1 receive the rows' k | v.  Bit for bit attn_decode per query."""
    who = "attn_decode_multi"
    R = S * T
    _req16(qkv, f"{who}.qkv")
    for t, nm in ((k_cache, "k_cache"), (v_cache, "v_cache"), (out, "out")):
        _req16(t, f"{who}.{nm}", like=qkv)
    _req(pos_rows, torch.int32, f"{who}.pos_rows")
    _need(qkv, R * (nq + 2 * nkv) * 64, f"{who}.qkv")
    _need(k_cache, S * kv_lmax * nkv * 64, f"{who}.k_cache")
    _need(v_cache, S * kv_lmax * nkv * 64, f"{who}.v_cache")
    _need(pos_rows, R, f"{who}.pos_rows")
    rows = R if out_layout == 0 else 8 if out_layout == 2 else 16 * ((R + 15) // 16)
    _need(out, rows * nq * 64, f"{who}.out")
    check(lib().tcavt_attn_decode_multi(ptr(qkv), ptr(k_cache), ptr(v_cache), ptr(pos_rows), ptr(out), S, T, nq, nkv, kv_lmax, scale,
                                        _DT[qkv.dtype], int(out_layout), stream_ptr()), "tcavt_attn_decode_multi")


def ngram_draft(history, hist_len, cur, pos, finished, k, max_matching_ngram_size, pad_token_id, n_draft, cur_rows, pos_rows):
    """Prompt-lookup draft of every sequence in one launch (tcavt_ngram_draft): from history int64 [S, cap] / hist_len and the
    per-slot state cur, pos, finished -> n_draft int32 [S], cur_rows int64 [S * (k + 1)], pos_rows int32 [S * (k + 1)]."""
    who = "ngram_draft"
    if history.dim() != 2:
        raise capi.TcavtError(f"{who}: history needs one row per sequence")
    S, T = history.shape[0], int(k) + 1
    _require(who, (history, torch.int64, S, "history"), (hist_len, torch.int32, S, "hist_len"), (cur, torch.int64, S, "cur"),
             (pos, torch.int32, S, "pos"), (finished, torch.int32, S, "finished"), (n_draft, torch.int32, S, "n_draft"),
             (cur_rows, torch.int64, S * T, "cur_rows"), (pos_rows, torch.int32, S * T, "pos_rows"))
    check(lib().tcavt_ngram_draft(ptr(history), history.shape[1], ptr(hist_len), ptr(cur), ptr(pos), ptr(finished), S, int(k),
                                  int(max_matching_ngram_size), int(pad_token_id), ptr(n_draft), ptr(cur_rows), ptr(pos_rows),
                                  stream_ptr()), "tcavt_ngram_draft")


def spec_verify_args(logits, T, n_draft, cur_rows, scratch, drafted, accepted, history, hist_len, params, step, max_new, out_row,
                     cur_tok, pos, finished, out_tokens, advance_pos=True, workspace=None, stop=None):
    """The tcavt_spec_verify_args of a verify-and-commit on logits fp32 [S * T, V] and the per-slot state of S sequences (the
    arguments of sample_tokens in its slots form), each tensor checked first.  scratch: int32 [S * T + S].  The struct names fixed
    device arrays: one serves every step of a call, captured or not."""
    who = "spec_verify"
    R, _ = logits.shape
    T = int(T)
    if history.dim() != 2 or out_tokens.dim() != 2 or T < 1 or R % T != 0 or history.shape[0] != R // T:
        raise capi.TcavtError(f"{who}: logits [S * T, V], history one row per sequence, out_tokens one row per request")
    S = R // T
    _sampler_guard(who, logits, workspace, S, S, 1, history, hist_len, step, cur_tok, pos, finished, out_tokens, slots=(max_new, out_row))
    _require(who, (n_draft, torch.int32, S, "n_draft"), (cur_rows, torch.int64, R, "cur_rows"), (scratch, torch.int32, R + S, "scratch"),
             (drafted, torch.int32, S, "drafted"), (accepted, torch.int32, S, "accepted"))
    sa = _sample_args(logits, R, S, history, hist_len, params, step, max_new, out_row, cur_tok, pos, finished, out_tokens, advance_pos,
                      workspace, stop)
    a = capi.SpecVerifyArgs()
    a.sample = ctypes.pointer(sa)
    a.n_draft, a.cur_rows, a.slot_of_row = n_draft.data_ptr(), cur_rows.data_ptr(), scratch.data_ptr()
    a.drafted, a.accepted, a.S, a.T = drafted.data_ptr(), accepted.data_ptr(), S, T
    a._keep = (sa, params, stop, logits, n_draft, cur_rows, scratch, drafted, accepted, history, hist_len, step, max_new, out_row,
               cur_tok, pos, finished, out_tokens, workspace)
    return a


def spec_verify(args):
    """T passes of (gate, sample_tokens) that select, compare with the draft and commit (tcavt_spec_verify); args: spec_verify_args."""
    check(lib().tcavt_spec_verify(ctypes.byref(args), stream_ptr()), "tcavt_spec_verify")


def tlayer_stack_forward(args):
    """args: capi.TStackArgs filled by tlayers._TLayerRunner.run_stack (which owns and sizes every buffer)."""
    check(lib().tcavt_tlayer_stack_forward(ctypes.byref(args), stream_ptr()), "tcavt_tlayer_stack_forward")


def cross_attn_forward(args):
    """args: capi.CrossAttnArgs filled by ltsf.TransformerLTSF.forward (which owns and sizes every buffer)."""
    check(lib().tcavt_cross_attn_forward(ctypes.byref(args), stream_ptr()), "tcavt_cross_attn_forward")


def cross_attn_backward(args):
    """args: capi.CrossAttnBwdArgs filled by backward.Backward._xattn_absorbed."""
    check(lib().tcavt_cross_attn_backward(ctypes.byref(args), stream_ptr()), "tcavt_cross_attn_backward")


def ltsf_forward(args, phase):
    """args: capi.LtsfArgs filled by ltsf.TransformerLTSF (which owns and sizes every buffer); phase 1 / 2 / 3."""
    check(lib().tcavt_ltsf_forward(ctypes.byref(args), int(phase), stream_ptr()), "tcavt_ltsf_forward")


def tlayer_stack_backward(args):
    """args: capi.TStackBwdArgs filled by backward.Backward.polygon (fp32 encoder layers)."""
    check(lib().tcavt_tlayer_stack_backward(ctypes.byref(args), stream_ptr()), "tcavt_tlayer_stack_backward")


def ltsf_backward(args, phase):
    """args: capi.LtsfBwdArgs filled by backward.Backward._ltsf_stage; phase 1 (head .. g_poly) / 2 (the rest) / 3."""
    check(lib().tcavt_ltsf_backward(ctypes.byref(args), int(phase), stream_ptr()), "tcavt_ltsf_backward")


def allreduce_flat(buf, nccl_comm):
    """In-place SUM all-reduce of a flat fp32 buffer on a raw RCCL communicator (an ncclComm_t as int / c_void_p) and the
    current stream: tcavt_allreduce_flat, the C host's form of the gradient-bucket exchange (Trainer itself goes through
    torch.distributed, whose process group owns its communicator)."""
    _req(buf, torch.float32, "allreduce_flat.buf")
    comm = nccl_comm if isinstance(nccl_comm, ctypes.c_void_p) else ctypes.c_void_p(int(nccl_comm) if nccl_comm else None)
    check(lib().tcavt_allreduce_flat(ptr(buf), buf.numel(), comm, stream_ptr()), "tcavt_allreduce_flat")
    return buf


def rmsnorm16(x16, gamma, eps, out16=None, out_f32=None):
    """RMSNorm of 16-bit rows (the final norm of the 16-bit residual stream): out16 and / or out_f32."""
    _req16(x16, "rmsnorm16.x16")
    _req(gamma, torch.float32, "rmsnorm16.gamma")
    M, H = x16.shape
    _need(gamma, H, "rmsnorm16.gamma")
    if out16 is None and out_f32 is None:
        out_f32 = torch.empty((M, H), dtype=torch.float32, device=x16.device)
    if out16 is not None:
        _req16(out16, "rmsnorm16.out16", like=x16)
        _need(out16, M * H, "rmsnorm16.out16")
    if out_f32 is not None:
        _req(out_f32, torch.float32, "rmsnorm16.out_f32")
        _need(out_f32, M * H, "rmsnorm16.out_f32")
    check(lib().tcavt_rmsnorm16(ptr(x16), ptr(gamma), eps, ptr(out16), ptr(out_f32), M, H, _DT[x16.dtype], stream_ptr()),
          "tcavt_rmsnorm16")
    return out16 if out_f32 is None else out_f32


def rownorm_prep(x, x16, part, npart=None, rounded_sums=False, stream_scale=1.0):
    """x16 = 16-bit copy of x [M, H]; part [M, npart] = (row's sum of squares, 0, ...): inputs of a fused RMSNorm.
    rounded_sums: sums of the rounded values (16-bit residual stream)."""
    _req(x, torch.float32, "rownorm_prep.x")
    _req16(x16, "rownorm_prep.x16")
    _req(part, torch.float32, "rownorm_prep.part")
    M, H = x.shape
    npart = npart or H // 64
    _need(x16, M * H, "rownorm_prep.x16")
    _need(part, M * npart, "rownorm_prep.part")
    check(lib().tcavt_rownorm_prep(ptr(x), ptr(x16), ptr(part), M, H, npart, _DT[x16.dtype], int(bool(rounded_sums)), float(stream_scale),
                                   stream_ptr()),
          "tcavt_rownorm_prep")


class StackEvents:
    """hipEvents for the in-situ kernel timing of tcavt_llama_stack_forward (10 per layer: start / stop around q|k|v,
    attention, o, gate|up, down)."""

    STAGES = ("qkv", "attn", "o", "gateup", "down")

    def __init__(self, n_layers):
        self.n = 10 * n_layers
        self.arr = (ctypes.c_void_p * self.n)()
        check(lib().tcavt_events_create(self.arr, self.n), "tcavt_events_create")

    def summary(self):
        """{stage: (launches, mean ms)} of the LAST pass recorded (call after a stream synchronise)."""
        out = {}
        for si, name in enumerate(self.STAGES):
            tot, cnt = 0.0, 0
            for li in range(self.n // 10):
                ms = ctypes.c_float(0.0)
                check(lib().tcavt_event_elapsed_ms(self.arr[li * 10 + 2 * si], self.arr[li * 10 + 2 * si + 1], ctypes.byref(ms)),
                      "tcavt_event_elapsed_ms")
                tot += ms.value
                cnt += 1
            out[name] = (cnt, tot / max(cnt, 1))
        return out

    def close(self):
        if self.arr is not None:
            lib().tcavt_events_destroy(self.arr, self.n)
            self.arr = None


# ---- LM loss on labels (csrc/lm_loss.hip): fused lm_head + cross-entropy, forward and backward ----------------------------
def lm_loss_workspace_bytes(rows, V, H):
    """Transient device memory of lm_loss_forward / lm_loss_backward for `rows` = B * L hidden-state rows."""
    return int(lib().tcavt_lm_loss_workspace_bytes(int(rows), int(V), int(H)))


def lm_table_t(table):
    """The backward's second operand: 16-bit [H, V rounded up to 64] transpose of the tied table, zero beyond V.  A layout of
    the frozen weights made once per checkpoint (LlamaWithCrossAttnPEFT.table_T caches it), not part of the workspace."""
    _req16(table, "lm_table_t.table")
    V, H = table.shape
    out = torch.zeros(H, (V + 63) // 64 * 64, dtype=table.dtype, device=table.device)
    out[:, :V].copy_(table.t())
    return out


def _lm_loss_args(h16, table, labels, Nq, B, L, kv_len, flag, workspace, who):
    _req16(h16, who + ".h16", rows_ok=True)
    _req16(table, who + ".table", like=h16)
    _req(labels, torch.int64, who + ".labels")
    _req(kv_len, torch.int32, who + ".kv_len")
    _req(flag, torch.int32, who + ".flag")
    _req(workspace, torch.uint8, who + ".workspace")
    if h16.dim() != 2 or table.dim() != 2 or h16.shape[1] != table.shape[1]:
        raise capi.TcavtError(f"{who}: h16 [rows, H] and table [V, H] required")
    V, H = table.shape
    if h16.shape[0] < B * L or labels.numel() != B * (L - Nq) or (kv_len is not None and kv_len.numel() < B):
        raise capi.TcavtError(f"{who}: h16 needs B * L rows, labels B * (L - Nq) elements, kv_len B")
    a = capi.LmLossArgs()
    a.h16, a.ldh, a.table = h16.data_ptr(), h16.stride(0), table.data_ptr()
    a.labels = labels.data_ptr()
    a.kv_len = None if kv_len is None else kv_len.data_ptr()
    a.B, a.L, a.V, a.H, a.Nq = B, L, V, H, Nq
    a.dtype16 = _DT[h16.dtype]
    a.flag = None if flag is None else flag.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
    return a


def lm_loss_forward(h16, table, labels, Nq, B, L, *, loss, count, lse, workspace, row_loss=None, kv_len=None, flag=None):
    """Mean cross-entropy of the labelled rows (include/tcavt.h: tcavt_lm_loss_forward).  h16: 16-bit [>= B * L, H]
    post-final-norm hidden states; table 16-bit [V, H]; labels int64 [B, L - Nq].  Writes loss fp32 [1], count int32 [1],
    lse (and row_loss) fp32 [B * L]; no host sync."""
    a = _lm_loss_args(h16, table, labels, Nq, B, L, kv_len, flag, workspace, "lm_loss_forward")
    for t, n, nm in ((loss, 1, "loss"), (lse, B * L, "lse"), (row_loss, B * L, "row_loss")):
        _req(t, torch.float32, "lm_loss_forward." + nm)
        _need(t, n, "lm_loss_forward." + nm)
    _req(count, torch.int32, "lm_loss_forward.count")
    a.loss, a.count, a.lse = loss.data_ptr(), count.data_ptr(), lse.data_ptr()
    a.row_loss = None if row_loss is None else row_loss.data_ptr()
    check(lib().tcavt_lm_loss_forward(ctypes.byref(a), stream_ptr()), "tcavt_lm_loss_forward")
    return loss


def lm_loss_backward(h16, table, table_t, labels, Nq, B, L, *, lse, count, g_out, workspace, g_loss=None, kv_len=None, flag=None):
    """g_out [B * L, H] (16-bit, its own dtype: bf16 for LoraBackward.run) = (g_loss / N) (softmax(z) - onehot) . table on the
    labelled rows, zeros elsewhere (tcavt_lm_loss_backward).  lse / count: as lm_loss_forward left them; table_t: lm_table_t."""
    a = _lm_loss_args(h16, table, labels, Nq, B, L, kv_len, flag, workspace, "lm_loss_backward")
    _req16(table_t, "lm_loss_backward.table_t", like=table)
    _req16(g_out, "lm_loss_backward.g_out", rows_ok=True)
    _req(lse, torch.float32, "lm_loss_backward.lse")
    _req(count, torch.int32, "lm_loss_backward.count")
    _req(g_loss, torch.float32, "lm_loss_backward.g_loss")
    _need(lse, B * L, "lm_loss_backward.lse")
    V, H = table.shape
    if table_t.dim() != 2 or table_t.shape[0] != H or g_out.dim() != 2 or g_out.shape[0] < B * L or g_out.shape[1] != H:
        raise capi.TcavtError("lm_loss_backward: table_t [H, >= V rounded up to 64] and g_out [>= B * L, H] required")
    a.table_t, a.ldt = table_t.data_ptr(), table_t.stride(0)
    a.lse, a.count = lse.data_ptr(), count.data_ptr()
    a.g_loss = None if g_loss is None else g_loss.data_ptr()
    a.g_out, a.ldg, a.grad_dtype = g_out.data_ptr(), g_out.stride(0), _DT[g_out.dtype]
    check(lib().tcavt_lm_loss_backward(ctypes.byref(a), stream_ptr()), "tcavt_lm_loss_backward")
    return g_out


def lm_eval_workspace_bytes(rows, V, H):
    """Transient device memory of lm_eval for `rows` = B * L hidden-state rows: row arrays and per-tile statistics only."""
    return int(lib().tcavt_lm_eval_workspace_bytes(int(rows), int(V), int(H)))


def lm_eval(h16, table, labels, Nq, B, L, *, loss, count, lse, pred, workspace, row_loss=None, correct=None, sample_tokens=None,
            sample_correct=None, sample_nll=None, kv_len=None, flag=None):
    """Teacher-forced evaluation pass (include/tcavt.h: tcavt_lm_eval): what lm_loss_forward writes, bit for bit, plus
    pred int32 [B * L] (arg-max column of every labelled row's logits, -1 elsewhere), correct int32 [1], sample_tokens /
    sample_correct int32 [B] and sample_nll fp32 [B].  Same operands and checks as lm_loss_forward; no host sync."""
    who = "lm_eval"
    _req16(h16, who + ".h16", rows_ok=True)
    _req16(table, who + ".table", like=h16)
    _req(labels, torch.int64, who + ".labels")
    _req(kv_len, torch.int32, who + ".kv_len")
    _req(flag, torch.int32, who + ".flag")
    _req(workspace, torch.uint8, who + ".workspace")
    if h16.dim() != 2 or table.dim() != 2 or h16.shape[1] != table.shape[1]:
        raise capi.TcavtError(f"{who}: h16 [rows, H] and table [V, H] required")
    V, H = table.shape
    if h16.shape[0] < B * L or labels.numel() != B * (L - Nq) or (kv_len is not None and kv_len.numel() < B):
        raise capi.TcavtError(f"{who}: h16 needs B * L rows, labels B * (L - Nq) elements, kv_len B")
    for t, n, nm in ((loss, 1, "loss"), (lse, B * L, "lse"), (row_loss, B * L, "row_loss"), (sample_nll, B, "sample_nll")):
        _req(t, torch.float32, who + "." + nm)
        _need(t, n, who + "." + nm)
    for t, n, nm in ((count, 1, "count"), (pred, B * L, "pred"), (correct, 1, "correct"), (sample_tokens, B, "sample_tokens"),
                     (sample_correct, B, "sample_correct")):
        _req(t, torch.int32, who + "." + nm)
        _need(t, n, who + "." + nm)
    if loss is None or count is None or lse is None or pred is None:
        raise capi.TcavtError(f"{who}: loss, count, lse and pred are required")
    a = capi.LmEvalArgs()
    a.h16, a.ldh, a.table = h16.data_ptr(), h16.stride(0), table.data_ptr()
    a.labels = labels.data_ptr()
    a.kv_len = None if kv_len is None else kv_len.data_ptr()
    a.B, a.L, a.V, a.H, a.Nq = B, L, V, H, Nq
    a.dtype16 = _DT[h16.dtype]
    a.loss, a.count, a.lse, a.pred = loss.data_ptr(), count.data_ptr(), lse.data_ptr(), pred.data_ptr()
    capi.bind(a, row_loss=row_loss, flag=flag, correct=correct, sample_tokens=sample_tokens, sample_correct=sample_correct,
              sample_nll=sample_nll)
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
    check(lib().tcavt_lm_eval(ctypes.byref(a), stream_ptr()), "tcavt_lm_eval")
    return pred
