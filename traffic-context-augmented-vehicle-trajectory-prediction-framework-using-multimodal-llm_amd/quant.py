"""The FP8 weight format of the decode step (include/tcavt.h: tcavt_pack_weight8) in plain torch, on any device.

This is the definition the pack kernel is tested against: OCP e4m3fn codes of the rows of a 16-bit matrix, each row scaled
by a power of two, and the byte layout the skinny GEMM streams.  Nothing here is on a hot path.

    codes, k = quantize(w)            # uint8 [N, K], int32 [N]:  code = e4m3(w * 2^-k), k minimal with amax * 2^-k <= 448
    buf = pack(w)                     # uint8 [N * K + 4 N]: fragment-major codes, then the fp32 scales 2^k
    wq = dequantize(codes, k, dtype)  # the 16-bit matrix code * 2^k -- what the FP8 path multiplies by, exactly

"MX8" (tcavt_quant_mx8 / tcavt_gemm_mx8, the opt-in block-scaled MLP of the frozen decoder) is the OCP MXFP8-E4M3 layout with the
same scale rule applied per block of 32 along K instead of per row:

    codes, sb = quantize_mx(x)        # uint8 [R, K], uint8 [R, K / 32]: E8M0 scale bytes, byte = k + 127, value 2^k
    xq = dequantize_mx(codes, sb, dtype)  # code * 2^k, exact (float64 allowed)

"KV8" (tcavt_kv_store8 / tcavt_attn_decode8, the opt-in FP8 KV cache of the decode step) is quantize_mx of every cached 64-element
row of a kv head, stored head-major:

    codes, sb = kv8_quantize(kv16)    # [B, L, nkv * 64] -> uint8 [B, nkv, L, 64], uint8 [B, nkv, L, 2]
    kv = kv8_dequantize(codes, sb, dtype)  # back to [B, L, nkv * 64], exact (float64 allowed)
"""
import torch

E4M3_MAX = 448.0
NAN_CODE = 0x7F


def row_exponents(w):
    """int32 [N]: per row the smallest k with amax * 2^-k <= 448 (amax = the row's largest magnitude); 0 for an all-zero
    row and for a row with a non-finite element."""
    amax = w.detach().abs().amax(dim=1).double()
    m, e = torch.frexp(amax)  # amax = m * 2^e, m in [0.5, 1); 448 = 0.875 * 2^9
    k = torch.where(m <= 0.875, e - 9, e - 8)
    k = torch.where((amax == 0) | ~torch.isfinite(amax), torch.zeros_like(k), k)
    return k.to(torch.int32)


def quantize(w):
    """w: 16-bit [N, K].  Returns (codes uint8 [N, K], k int32 [N]): the e4m3fn value nearest to the exact product
    w * 2^-k, ties to even; the NaN code everywhere in a row that holds a non-finite element."""
    assert w.dim() == 2 and w.dtype in (torch.float16, torch.bfloat16)
    k = row_exponents(w)
    scaled = torch.ldexp(w.detach().float(), -k[:, None])  # exact: a 16-bit value times a power of two in fp32
    codes = scaled.to(torch.float8_e4m3fn).view(torch.uint8)
    bad = ~torch.isfinite(w.detach().float()).all(dim=1)
    codes = torch.where(bad[:, None], torch.full_like(codes, NAN_CODE), codes)
    return codes, k


def dequantize(codes, k, dtype):
    """code * 2^k as a `dtype` (fp16 / bf16) matrix [N, K]: exact whenever the product is a normal number of that type."""
    lut = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().to(codes.device)  # (the 256 values, decoded on the host)
    v = lut[codes.long()]
    return torch.ldexp(v, k[:, None].to(torch.int32)).to(dtype)


def pack_chunks(codes):
    """uint8 [N, K] -> uint8 [N * K] in the consuming wave's order: block b (16 rows), k-step j (32 columns) is the 512-byte
    chunk b * K / 32 + j; lane l = 16 q + r holds codes[16 b + r][32 j + 8 q : + 8] at byte 8 l."""
    N, K = codes.shape
    assert N % 16 == 0 and K % 32 == 0
    return codes.view(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1)


def unpack_chunks(flat, N, K):
    """Inverse of pack_chunks."""
    return flat.view(N // 16, K // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(N, K)


def scales(k):
    """fp32 [N]: exactly 2^k."""
    return torch.ldexp(torch.ones(k.shape, dtype=torch.float32, device=k.device), k.to(torch.int32))


def pack(w):
    """The whole buffer tcavt_pack_weight8 writes: uint8 [N * K + 4 N]."""
    codes, k = quantize(w)
    return torch.cat([pack_chunks(codes), scales(k).view(torch.uint8)])


def unpack(buf, N, K):
    """(codes uint8 [N, K], k int32 [N]) of a packed buffer."""
    codes = unpack_chunks(buf[: N * K], N, K)
    sc = buf[N * K:].contiguous().view(torch.float32)
    _, e = torch.frexp(sc)
    return codes, (e - 1).to(torch.int32)


def snap(w):
    """w rounded to the FP8 format and back, in w's own type: a matrix on which the FP8 and the 16-bit decode paths agree
    bit for bit.  fp16: anything below the smallest normal (2^-14) becomes zero, so that no product rests on how an MFMA
    treats subnormal operands."""
    codes, k = quantize(w)
    wq = dequantize(codes, k, w.dtype)
    if w.dtype == torch.float16:
        wq = torch.where(wq.abs() < 2.0 ** -14, torch.zeros_like(wq), wq)
    return wq


MX_BLOCK = 32
E8M0_BIAS = 127


def quantize_mx(x):
    """x: 16-bit [R, K], K % 32 == 0.  Returns (codes uint8 [R, K], scale bytes uint8 [R, K / 32]).  Per (row, block of 32 along K):
    k = row_exponents' rule on the block (the smallest k with amax * 2^-k <= 448), clamped to [-127, 127]; byte = k + 127;
    code = e4m3fn(x * 2^-k), nearest, ties to even (never saturates; below the clamp the codes underflow).  An all-zero block
    has k = 0; a block with a non-finite element has the NaN code throughout and scale byte 127."""
    assert x.dim() == 2 and x.dtype in (torch.float16, torch.bfloat16) and x.shape[1] % MX_BLOCK == 0
    R, K = x.shape
    xb = x.detach().reshape(R * (K // MX_BLOCK), MX_BLOCK)
    k = row_exponents(xb).clamp(-E8M0_BIAS, E8M0_BIAS)
    scaled = torch.ldexp(xb.double(), -k[:, None]).float()  # exact in float64; its fp32 image is exact or below every e4m3 step
    codes = scaled.to(torch.float8_e4m3fn).view(torch.uint8)
    bad = ~torch.isfinite(xb.float()).all(dim=1)
    codes = torch.where(bad[:, None], torch.full_like(codes, NAN_CODE), codes)
    return codes.reshape(R, K), (k + E8M0_BIAS).to(torch.uint8).reshape(R, K // MX_BLOCK)


def dequantize_mx(codes, scale_bytes, dtype):
    """code * 2^(byte - 127) as `dtype` (fp16 / bf16 / fp32 / float64) [R, K]: exact whenever the product is a number of that
    type (always in float64)."""
    lut = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double().to(codes.device)
    R, K = codes.shape
    v = lut[codes.long()].reshape(R, K // MX_BLOCK, MX_BLOCK)
    k = scale_bytes.to(torch.int32) - E8M0_BIAS
    return torch.ldexp(v, k[:, :, None]).reshape(R, K).to(dtype)


def snap_mx(x):
    """x rounded to the MX8 format and back, in x's own type (fp16: anything below the smallest normal becomes zero, as in
    `snap`)."""
    codes, sb = quantize_mx(x)
    xq = dequantize_mx(codes, sb, x.dtype)
    if x.dtype == torch.float16:
        xq = torch.where(xq.abs() < 2.0 ** -14, torch.zeros_like(xq), xq)
    return xq


KV_HEAD_DIM = 64


def kv8_quantize(kv16):
    """"KV8", the opt-in FP8 KV cache of the decode step (include/tcavt.h: tcavt_kv_store8 / tcavt_attn_decode8): a cached key or value
    row of one kv head (64 elements) is quantize_mx of that row -- 64 e4m3fn codes and 2 E8M0 scale bytes -- and the rows of one kv
    head are consecutive (head-major).  kv16: 16-bit [B, L, nkv * 64] (the 16-bit cache's token-major order).
    Returns (codes uint8 [B, nkv, L, 64], scale bytes uint8 [B, nkv, L, 2])."""
    assert kv16.dim() == 3 and kv16.shape[2] % KV_HEAD_DIM == 0
    B, L, w = kv16.shape
    nkv = w // KV_HEAD_DIM
    rows = kv16.detach().reshape(B, L, nkv, KV_HEAD_DIM).permute(0, 2, 1, 3).reshape(B * nkv * L, KV_HEAD_DIM)
    codes, sb = quantize_mx(rows)
    return codes.reshape(B, nkv, L, KV_HEAD_DIM), sb.reshape(B, nkv, L, KV_HEAD_DIM // MX_BLOCK)


def kv8_dequantize(codes, scale_bytes, dtype):
    """code * 2^(byte - 127) of a KV8 plane pair, back in token-major order: `dtype` (fp16 / bf16 / fp32 / float64) [B, L, nkv * 64]."""
    B, nkv, L, d = codes.shape
    assert d == KV_HEAD_DIM and tuple(scale_bytes.shape) == (B, nkv, L, KV_HEAD_DIM // MX_BLOCK)
    x = dequantize_mx(codes.reshape(B * nkv * L, d), scale_bytes.reshape(B * nkv * L, d // MX_BLOCK), dtype)
    return x.reshape(B, nkv, L, d).permute(0, 2, 1, 3).reshape(B, L, nkv * d)
