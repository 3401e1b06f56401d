// Backward of the decoder layers for the LoRA-trainable variant (SURVEY.md 8f.1;
// modify_scripts/modify_train.py:512-528 trains lora_A / lora_B of q_proj, v_proj while every base weight stays frozen):
// the activation gradient walks back through all layers -- dgrad GEMMs against transposed copies of the frozen
// weights (gemm_bf16.hip), the attention backward (attn_bwd.hip; its cross-check forms: attn_bwd_check.hip), and the
// pointwise / row / weight-gradient pieces and the walk itself (tcavt_llama_stack_backward) here.
#include "common.hpp"
#include "philox.hpp"

namespace tcavt {

__device__ __forceinline__ float sigmoid_f(float g) { return __builtin_amdgcn_rcpf(1.f + __expf(-g)); }

template <bool F16>
__device__ __forceinline__ float half16(unsigned int w, int k) { return k ? from16_hi<F16>(w) : from16_lo<F16>(w); }

// gu: [M, 2I] bf16 in the interleaved layout of TCAVT_EPI_SILU_MUL (blocks of 16 gate columns, then the 16 up columns
// of the same features); g_act: [M, I] bf16 = dL/d(silu(gate) * up).  g_gu gets dL/dgate, dL/dup in the same layout.
template <bool F16>
__global__ __launch_bounds__(256) void silu_mul_bwd_kernel(const bf16_t* __restrict__ gu, const bf16_t* __restrict__ g_act,
                                                           bf16_t* __restrict__ g_gu, long M, int I) {
  // one thread per block of 16 features: 32 B of gate, 32 B of up (adjacent), 32 B of g_act
  const long blk = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long nblk = M * (I >> 4);
  if (blk >= nblk) return;
  const u32x4* src = reinterpret_cast<const u32x4*>(gu + blk * 32);
  const u32x4* dsrc = reinterpret_cast<const u32x4*>(g_act + blk * 16);
  u32x4 gv[2] = {src[0], src[1]}, uv[2] = {src[2], src[3]}, dv[2] = {dsrc[0], dsrc[1]};
  u32x4 og[2], ou[2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float r[2][2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const float g = half16<F16>(gv[h][e], k), u = half16<F16>(uv[h][e], k), d = half16<F16>(dv[h][e], k);
        const float sg = sigmoid_f(g);
        r[0][k] = d * u * sg * (1.f + g * (1.f - sg));
        r[1][k] = d * g * sg;
      }
      og[h][e] = pack16x2<F16>(r[0][0], r[0][1]);
      ou[h][e] = pack16x2<F16>(r[1][0], r[1][1]);
    }
  u32x4* dst = reinterpret_cast<u32x4*>(g_gu + blk * 32);
  dst[0] = og[0]; dst[1] = og[1]; dst[2] = ou[0]; dst[3] = ou[1];
}

// RMSNorm backward, one wave per row:  y = x * r * gamma,  r = rsqrt(mean(x^2) + eps)
//   gx = r * (gy*gamma) - x * r^3 * mean(gy*gamma*x)
// gy = gy_a (+ gy_b): the LoRA branch hands in its own gradient of the same normed row.  accumulate: gx += .
// GF16 / OF16: 16-bit type of the incoming gradients / of the outgoing 16-bit copy.  gy_scale (optional, device scalar):
// the incoming gradients are multiplied by it -- where the backward enters its power-of-two scale (tcavt_grad_scale_pick).
// XT: type of x -- 0 fp32, 1 fp16, 2 bf16 (the forward's 16-bit residual stream, kept per layer by the tape)
template <int XT>
__device__ __forceinline__ void load_x8(const void* xr, int c, f32x4& x0, f32x4& x1) {
  if constexpr (XT == 0) {
    const float* f = static_cast<const float*>(xr);
    x0 = *reinterpret_cast<const f32x4*>(f + c);
    x1 = *reinterpret_cast<const f32x4*>(f + c + 4);
  } else {
    const u32x4 v = *reinterpret_cast<const u32x4*>(static_cast<const bf16_t*>(xr) + c);
    x0 = f32x4{from16_lo<XT == 1>(v[0]), from16_hi<XT == 1>(v[0]), from16_lo<XT == 1>(v[1]), from16_hi<XT == 1>(v[1])};
    x1 = f32x4{from16_lo<XT == 1>(v[2]), from16_hi<XT == 1>(v[2]), from16_lo<XT == 1>(v[3]), from16_hi<XT == 1>(v[3])};
  }
}
template <bool GF16, bool OF16, int XT>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const void* __restrict__ x, const float* __restrict__ gamma,
                                                          const bf16_t* __restrict__ gy_a, const bf16_t* __restrict__ gy_b,
                                                          float eps, float* __restrict__ gx, bf16_t* __restrict__ gx_bf16,
                                                          int accumulate, int M, int H, const float* __restrict__ gy_scale) {
  const float gsc = gy_scale ? *gy_scale : 1.f;
  // H % 8 == 0: a lane handles 8 consecutive columns per step (2 x 16 B of x, 16 B of each gradient)
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const void* xr = XT == 0 ? static_cast<const void*>(static_cast<const float*>(x) + (long)row * H)
                           : static_cast<const void*>(static_cast<const bf16_t*>(x) + (long)row * H);
  const bf16_t* ga = gy_a + (long)row * H;
  const bf16_t* gb = gy_b ? gy_b + (long)row * H : nullptr;
  auto load_g = [&](int c, float (&g)[8]) {
    const u32x4 a = *reinterpret_cast<const u32x4*>(ga + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      g[2 * e] = from16_lo<GF16>(a[e]);
      g[2 * e + 1] = from16_hi<GF16>(a[e]);
    }
    if (gb) {
      const u32x4 b = *reinterpret_cast<const u32x4*>(gb + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        g[2 * e] += from16_lo<GF16>(b[e]);
        g[2 * e + 1] += from16_hi<GF16>(b[e]);
      }
    }
    const f32x4 w0 = *reinterpret_cast<const f32x4*>(gamma + c) * gsc, w1 = *reinterpret_cast<const f32x4*>(gamma + c + 4) * gsc;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      g[e] *= w0[e];
      g[4 + e] *= w1[e];
    }
  };
  float ss = 0.f, dot = 0.f;
  for (int c = lane * 8; c < H; c += 512) {
    float g[8];
    load_g(c, g);
    f32x4 x0, x1;
    load_x8<XT>(xr, c, x0, x1);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      ss = fmaf(x0[e], x0[e], ss);
      ss = fmaf(x1[e], x1[e], ss);
      dot = fmaf(g[e], x0[e], dot);
      dot = fmaf(g[4 + e], x1[e], dot);
    }
  }
  ss = wave_sum(ss);
  dot = wave_sum(dot);
  const float r = rsqrtf(ss / (float)H + eps);
  const float k = dot / (float)H * r * r * r;
  float* o = gx + (long)row * H;
  for (int c = lane * 8; c < H; c += 512) {
    float g[8];
    load_g(c, g);
    f32x4 x0, x1;
    load_x8<XT>(xr, c, x0, x1);
    f32x4 v0, v1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v0[e] = r * g[e] - x0[e] * k;
      v1[e] = r * g[4 + e] - x1[e] * k;
    }
    if (accumulate) {
      const f32x4 p0 = *reinterpret_cast<const f32x4*>(o + c), p1 = *reinterpret_cast<const f32x4*>(o + c + 4);
      v0 += p0;
      v1 += p1;
    }
    *reinterpret_cast<f32x4*>(o + c) = v0;
    *reinterpret_cast<f32x4*>(o + c + 4) = v1;
    if (gx_bf16) {
      u32x4 b = {pack16x2<OF16>(v0[0], v0[1]), pack16x2<OF16>(v0[2], v0[3]), pack16x2<OF16>(v1[0], v1[1]), pack16x2<OF16>(v1[2], v1[3])};
      *reinterpret_cast<u32x4*>(gx_bf16 + (long)row * H + c) = b;
    }
  }
}

// ---------------------------------------------------------------------------
// torch.nn.utils.clip_grad_norm_(params, max_norm) on the flat gradient vector (modify_scripts/modify_train.py:1192), without
// a host round trip and with a fixed summation order: 1024 block partials of sum(g^2), one block adds them in index order
// and leaves  grad_scale * min(1, max_norm / (norm + 1e-6))  in scratch[1024] (norm = grad_scale * ||g|| in scratch[1025]),
// a third launch scales g.  grad_scale = 1 / world turns the SUM-all-reduced gradient of a data-parallel step into the
// DDP-averaged one FIRST, so that the threshold applies to the gradient the reference clips (modify_train.py:1192 clips
// after DDP's averaging all-reduce).
// ---------------------------------------------------------------------------
constexpr int CLIP_BLOCKS = 1024;
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ g, long n, float* __restrict__ part) {
  __shared__ float sh[4];
  const long per = (n + CLIP_BLOCKS - 1) / CLIP_BLOCKS;
  const long lo = (long)blockIdx.x * per, hi = min(lo + per, n);
  float a = 0.f;
  for (long i = lo + threadIdx.x; i < hi; i += 256) a = fmaf(g[i], g[i], a);
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__global__ __launch_bounds__(64) void clip_scale_kernel(float* __restrict__ part, float max_norm, float grad_scale) {
  float a = 0.f;
  for (int i = threadIdx.x; i < CLIP_BLOCKS; i += 64) a += part[i];  // lane l: partials l, l + 64, ... in order
  a = wave_sum(a);
  if (threadIdx.x == 0) {
    const float norm = grad_scale * sqrtf(a);
    part[CLIP_BLOCKS] = grad_scale * fminf(1.f, max_norm / (norm + 1e-6f));
    part[CLIP_BLOCKS + 1] = norm;
  }
}
__global__ __launch_bounds__(256) void scale_by_kernel(float* __restrict__ g, long n, const float* __restrict__ scale) {
  const float sc = *scale;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) g[i] *= sc;
}

// 1 / rms of a token from the fused RMSNorm's partial sums of squares, added in index order (as row_rscale of the GEMMs)
__device__ __forceinline__ float part_rscale(const float* __restrict__ q, int npart, float inv_h, float eps) {
  float ss = 0.f;
  for (int i = 0; i < npart; i += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(q + i);
    ss += v[0];
    ss += v[1];
    ss += v[2];
    ss += v[3];
  }
  return rsqrtf(ss * inv_h + eps);
}

// ---------------------------------------------------------------------------
// dA of both adapters in ONE pass over the taped residual stream (LoRA-trainable variant):
//     dA_q[r][n] = gamma[n] * sum_m g_t[m][r] * drop_q(rs[m] h[m][n]),   dA_v likewise with g_t[m][16 + r] and drop_v
// h = the layer's 16-bit input stream, rs = 1 / rms of its rows (from the forward's partial sums), gamma = the input
// norm's gain, drop = the forward's masks regenerated (Philox, one call per octet and site) -- i.e. g_t^T (mask * rmsnorm(h))
// without ever writing rmsnorm(h), its two dropped copies or reading them back (round 3 before this: one norm kernel, two mask
// kernels and two wgrad_tn launches per layer, ~230 MB of traffic instead of 33).  Layout of the work as wgrad_tn_kernel:
// a workgroup owns 256 columns and a range of tokens, stages 32 tokens per step transposed in LDS (two tokens per dword),
// partial sums meet in dA through fp32 atomics.
// ---------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(256) void lora_wgrad_a_kernel(const bf16_t* __restrict__ X, const float* __restrict__ part, int npart,
                                                           float inv_h, float eps, const float* __restrict__ gamma,
                                                           const bf16_t* __restrict__ Gt, float* __restrict__ dA, long ldc, int M,
                                                           int H, int m_per_wg, DropoutP dq, DropoutP dv) {
  constexpr int XS = 40;
  __shared__ __attribute__((aligned(16))) bf16_t xq[256 * XS];
  __shared__ __attribute__((aligned(16))) bf16_t xv[256 * XS];
  __shared__ __attribute__((aligned(16))) bf16_t gt[32 * XS];
  // 1 / rms of the 32 tokens of a step.  It goes to the STREAM operand (rs h: rms 1 whatever the layer), not to g_t: the
  // gradient operand sits under the backward's power-of-two scale near the top of the half range, and 1 / rms of the
  // embedding rows layer 0 reads is ~50 -- g_t rs left the range there (inf, then NaN in the product)
  __shared__ float rs_s[32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h0 = blockIdx.x * 256;
  const int mbeg = blockIdx.y * m_per_wg, mend = min(mbeg + m_per_wg, M);
  const int r16 = lane & 15, kq = lane >> 4;
  const bool drop = dq.p > 0.f;
  const bf16_t* xvp = drop ? xv : xq;
  f32x4 acc[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int tp = tid >> 4, cc = (tid & 15) * 16;  // this thread stages tokens 2 tp, 2 tp + 1, columns cc .. cc + 15
  const int grow = tid >> 2, gc0 = (tid & 3) * 8;  // ... and (tid < 128) token grow, g_t columns gc0 .. gc0 + 7
  for (int m0 = mbeg; m0 < mend; m0 += 32) {
    {
      u32x4 v[2][2];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int m = m0 + 2 * tp + r;
#pragma unroll
        for (int o = 0; o < 2; ++o) {
          v[r][o] = u32x4{0u, 0u, 0u, 0u};
          if (m < mend && h0 + cc + 8 * o < H) v[r][o] = *reinterpret_cast<const u32x4*>(X + (long)m * H + h0 + cc + 8 * o);
        }
      }
      u32x4 gv = {0u, 0u, 0u, 0u};
      if (tid < 128 && m0 + grow < mend) gv = *reinterpret_cast<const u32x4*>(Gt + (long)(m0 + grow) * 64 + gc0);
      if (tid < 32) rs_s[tid] = m0 + tid < mend ? part_rscale(part + (long)(m0 + tid) * npart, npart, inv_h, eps) : 0.f;
      __syncthreads();
      const float rs2[2] = {rs_s[2 * tp], rs_s[2 * tp + 1]};
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        u32x4 wq[2], wv[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          float sq[8], sv[8];
          if (drop) {  // (uniform) the forward's masks: element (m, n) of site q / v, one generator call per octet
            const unsigned long long oct =
                ((unsigned long long)(m0 + 2 * tp + r) * (unsigned long long)H + (unsigned long long)(h0 + cc + 8 * o)) >> 3;
            dropout_oct(dq, oct, sq);
            dropout_oct(dv, oct, sv);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float lo = from16_lo<F16>(v[r][o][e]) * rs2[r], hi = from16_hi<F16>(v[r][o][e]) * rs2[r];
            wq[r][e] = drop ? pack16x2<F16>(lo * sq[2 * e], hi * sq[2 * e + 1]) : pack16x2<F16>(lo, hi);
            if (drop) wv[r][e] = pack16x2<F16>(lo * sv[2 * e], hi * sv[2 * e + 1]);
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {  // columns cc + 8 o + 2 e (+ 1): tokens 2 tp | 2 tp + 1 in one dword
          const int c = cc + 8 * o + 2 * e;
          *reinterpret_cast<unsigned int*>(&xq[c * XS + 2 * tp]) = (wq[0][e] & 0xffffu) | (wq[1][e] << 16);
          *reinterpret_cast<unsigned int*>(&xq[(c + 1) * XS + 2 * tp]) = (wq[0][e] >> 16) | (wq[1][e] & 0xffff0000u);
          if (drop) {
            *reinterpret_cast<unsigned int*>(&xv[c * XS + 2 * tp]) = (wv[0][e] & 0xffffu) | (wv[1][e] << 16);
            *reinterpret_cast<unsigned int*>(&xv[(c + 1) * XS + 2 * tp]) = (wv[0][e] >> 16) | (wv[1][e] & 0xffff0000u);
          }
        }
      }
      if (tid < 128) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          gt[(gc0 + 2 * e) * XS + grow] = static_cast<bf16_t>(gv[e] & 0xffffu);
          gt[(gc0 + 2 * e + 1) * XS + grow] = static_cast<bf16_t>(gv[e] >> 16);
        }
      }
    }
    __syncthreads();
    // wave: columns h0 + 64 wave .. + 63; A = g_t^T rows (q adapter: 0..15, v adapter: 16..31), B = masked (rs h)^T rows, K = 32 tokens
    const u32x4 aq = *reinterpret_cast<const u32x4*>(&gt[r16 * XS + kq * 8]);
    const u32x4 av = *reinterpret_cast<const u32x4*>(&gt[(16 + r16) * XS + kq * 8]);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int row = (wave * 64 + b * 16 + r16) * XS + kq * 8;
      const u32x4 bq = *reinterpret_cast<const u32x4*>(&xq[row]);
      const u32x4 bv = *reinterpret_cast<const u32x4*>(&xvp[row]);
      acc[0][b] = mfma16b<F16>(__builtin_bit_cast(bf16x8, aq), __builtin_bit_cast(bf16x8, bq), acc[0][b]);
      acc[1][b] = mfma16b<F16>(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv), acc[1][b]);
    }
    __syncthreads();
  }
  // acc[a][b]: adapter a, rank row 4 kq + e, column h0 + 64 wave + 16 b + r16
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int h = h0 + wave * 64 + b * 16 + r16;
      if (h >= H) continue;
      const float gm = gamma[h];
#pragma unroll
      for (int e = 0; e < 4; ++e) atomicAdd(dA + (long)(a * 16 + 4 * kq + e) * ldc + h, acc[a][b][e] * gm);
    }
}

// ---------------------------------------------------------------------------
// Weight gradient with a SKINNY output, without physical transposes:
//     C[n][h] (+)= sum_m G[m][g0 + n] * X[m][h]          n < 16 * NB (NB <= 4),  h < H,  contraction over the M tokens
// (LoRA: dA = g_t^T x with n = 16 per adapter, dB^T = t^T g_qkv with n = 32).  Both operands are token-major, so the
// MFMA's K index (the token) runs DOWN their rows; round 1 transposed both with tcavt_transpose16 first (a 32 MB read +
// write per operand and layer).  Here a workgroup stages 32 tokens x 256 columns of X and 32 x 16 NB of G per step and
// writes them into LDS already transposed ([column][token], 16-bit scattered stores), so the fragments are plain
// 16-byte row reads; X is read exactly once.  The token range is split over gridDim.y workgroups, whose partial sums
// meet in C through fp32 atomics (C zeroed or holding an earlier contribution; same reproducibility class as the other
// weight gradients: up to the float summation order).  trans_out: store C^T ([h][ldc] layout) instead.
// ---------------------------------------------------------------------------
// GF16: G (and then X as well) is IEEE half and the products run on the f16 MFMA; otherwise G is bf16 and an fp16 X
// (XF16: a forward activation of the fp16 storage contract) is converted while it is staged
template <bool XF16, bool GF16 = false>
__global__ __launch_bounds__(256) void wgrad_tn_kernel(const bf16_t* __restrict__ G, long ldg, int g0, int NB,
                                                       const bf16_t* __restrict__ X, long ldx, float* __restrict__ C,
                                                       long ldc, int M, int H, int m_per_wg, int trans_out,
                                                       const float* __restrict__ rs_part, int rs_npart, float rs_inv_h,
                                                       float rs_eps) {
  // rs_part (optional): G's rows are multiplied by 1 / rms of their token while they are staged -- the fused RMSNorm's partial
  // sums of squares [M][rs_npart], added in index order as the forward's GEMMs do (dB of the adapters: the tape holds the
  // un-normalised t, the graph's t is rs * t)
  constexpr int XS = 40;  // LDS row stride in 16-bit elements (32 tokens + pad; 80 bytes: 16-byte aligned rows)
  __shared__ __attribute__((aligned(16))) bf16_t xt[256 * XS];
  __shared__ __attribute__((aligned(16))) bf16_t gt[64 * XS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h0 = blockIdx.x * 256;
  const int mbeg = blockIdx.y * m_per_wg, mend = min(mbeg + m_per_wg, M);
  const int r16 = lane & 15, kq = lane >> 4;
  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int xrow = tid >> 3, xc0 = (tid & 7) * 32;  // this thread stages token xrow, columns xc0 .. xc0 + 31
  const int grow = tid >> 3, gc0 = (tid & 7) * 8;   // ... and token grow, G columns gc0 .. gc0 + 7 (when < 16 NB)
  for (int m0 = mbeg; m0 < mend; m0 += 32) {
    {
      const int m = m0 + xrow;
      const bool ok = m < mend;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        u32x4 v = {0u, 0u, 0u, 0u};
        const int col = h0 + xc0 + c * 8;
        if (ok && col < H) v = *reinterpret_cast<const u32x4*>(X + (long)m * ldx + col);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          bf16_t lo = static_cast<bf16_t>(v[e] & 0xffffu), hi = static_cast<bf16_t>(v[e] >> 16);
          if constexpr (XF16 && !GF16) {  // forward activation in fp16, gradient operand in bf16: one type for the MFMA
            lo = f32_to_bf16(f16_to_f32(lo));
            hi = f32_to_bf16(f16_to_f32(hi));
          }
          xt[(xc0 + c * 8 + 2 * e) * XS + xrow] = lo;
          xt[(xc0 + c * 8 + 2 * e + 1) * XS + xrow] = hi;
        }
      }
      if (gc0 < 16 * NB) {
        u32x4 v = {0u, 0u, 0u, 0u};
        const int mg = m0 + grow;
        if (mg < mend) v = *reinterpret_cast<const u32x4*>(G + (long)mg * ldg + g0 + gc0);
        if (rs_part && mg < mend) {
          const float rs = part_rscale(rs_part + (long)mg * rs_npart, rs_npart, rs_inv_h, rs_eps);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = pack16x2<GF16>(from16_lo<GF16>(v[e]) * rs, from16_hi<GF16>(v[e]) * rs);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          gt[(gc0 + 2 * e) * XS + grow] = static_cast<bf16_t>(v[e] & 0xffffu);
          gt[(gc0 + 2 * e + 1) * XS + grow] = static_cast<bf16_t>(v[e] >> 16);
        }
      }
    }
    __syncthreads();
    // wave: columns h0 + 64 wave .. + 63 (four 16-column blocks); A = G^T rows (n), B = X^T rows (h), K = 32 tokens
    u32x4 bf[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) bf[b] = *reinterpret_cast<const u32x4*>(&xt[(wave * 64 + b * 16 + r16) * XS + kq * 8]);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      if (a < NB) {
        const u32x4 af = *reinterpret_cast<const u32x4*>(&gt[(a * 16 + r16) * XS + kq * 8]);
#pragma unroll
        for (int b = 0; b < 4; ++b)
          acc[a][b] = mfma16b<GF16>(__builtin_bit_cast(bf16x8, af), __builtin_bit_cast(bf16x8, bf[b]), acc[a][b]);
      }
    }
    __syncthreads();
  }
  // acc[a][b]: rows n = 16 a + 4 kq .. + 3, column h = h0 + 64 wave + 16 b + r16
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    if (a >= NB) continue;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int h = h0 + wave * 64 + b * 16 + r16;
      if (h >= H) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = a * 16 + 4 * kq + e;
        float* dst = trans_out ? C + (long)h * ldc + n : C + (long)n * ldc + h;
        atomicAdd(dst, acc[a][b][e]);
      }
    }
  }
}

// The four adapter gradients of one layer leave the two scratch matrices (dA [64][H]: rows 0.. = A_q, 16.. = A_v; dB [nqkv][64]:
// q rows x columns 0.., v rows x columns 16..) for the caller's tensors, times *scale, in ONE launch that also zeroes the
// scratch for the next layer's atomically accumulated sums (was: two memsets + four scale-and-copy launches per layer on the
// leaf queue, 96 launches per step).
__global__ __launch_bounds__(256) void adapter_grads_out_kernel(float* __restrict__ dA, float* __restrict__ dB, float* __restrict__ gAq,
                                                                float* __restrict__ gAv, float* __restrict__ gBq, float* __restrict__ gBv,
                                                                int H, int nqkv, int q_rows, int v_row0, int r,
                                                                const float* __restrict__ scale) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long nA = (long)64 * H;
  const float sc = scale ? *scale : 1.f;
  if (idx < nA) {
    const int i = (int)(idx / H), j = (int)(idx - (long)i * H);
    const float v = dA[idx];
    dA[idx] = 0.f;
    if (i < r) gAq[(long)i * H + j] = v * sc;
    else if (i >= 16 && i < 16 + r) gAv[(long)(i - 16) * H + j] = v * sc;
    return;
  }
  const long k = idx - nA;
  if (k >= (long)nqkv * 64) return;
  const int i = (int)(k >> 6), j = (int)(k & 63);
  const float v = dB[k];
  dB[k] = 0.f;
  if (i < q_rows && j < r) gBq[(long)i * r + j] = v * sc;
  else if (i >= v_row0 && j >= 16 && j < 16 + r) gBv[(long)(i - v_row0) * r + (j - 16)] = v * sc;
}

// ---------------------------------------------------------------------------
// Power-of-two scale of the fp16 backward: S = 2^k with  max|g| * S  in [target / 2, target]  (g = the 16-bit gradient(s) the
// backward starts from; bf16, so they cannot overflow themselves).  The backward is linear in g: every 16-bit gradient
// tensor downstream carries the factor S, the fp32 weight gradients are multiplied by 1 / S at the end.  Decided on the
// device (no host synchronisation): scale[0] = S, scale[1] = 1 / S.  All-zero g, or an inf in g: S = 1.  A NaN is dropped by
// the maximum (fmaxf), so S follows the finite values beside it (S = 1 if there are none).  Either way the non-finite
// gradient itself walks on and reaches the gated optimizer as it did before.  The exponent of S is clamped to +-60.
// ---------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(256) void grad_amax_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ b, long n8,
                                                        unsigned int* __restrict__ amax_bits) {
  float m = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const u32x4 v = reinterpret_cast<const u32x4*>(a)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) m = fmaxf(m, fmaxf(fabsf(from16_lo<F16>(v[e])), fabsf(from16_hi<F16>(v[e]))));
    if (b) {
      const u32x4 w = reinterpret_cast<const u32x4*>(b)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) m = fmaxf(m, fmaxf(fabsf(from16_lo<F16>(w[e])), fabsf(from16_hi<F16>(w[e]))));
    }
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(amax_bits, __float_as_uint(m));  // (non-negative floats order as their bits; NaN is dropped by fmaxf)
}
__global__ void grad_scale_set_kernel(unsigned int* __restrict__ amax_bits, float target, float* __restrict__ scale,
                                      const int* __restrict__ backoff) {
  const float m = __uint_as_float(*amax_bits);
  float s = 1.f;
  if (m > 0.f && m < 3.0e38f) {
    const float q = target / m;
    int e;
    // a quotient that left fp32 (bf16 gradients below ~2^-120: inf, for which frexpf leaves e = 0 and S came out as 1 / 2; or 0)
    // ends at the clamp below, like every other quotient beyond 2^+-60
    if (q > 3.0e38f) e = 200;
    else if (q < 1.2e-38f) e = -200;
    else (void)frexpf(q, &e);           // target / m = f * 2^e, f in [0.5, 1)
    // backoff (tcavt_adamw_gated's ctl[6]): binary orders of extra headroom, raised by four whenever an update was skipped for
    // a non-finite gradient norm -- the walk grew the gradient by more than the 2^8 the target leaves -- and given back slowly
    e = max(-60, min(60, e - 1 - (backoff ? *backoff : 0)));       // 2^(e-1) <= target / m
    s = ldexpf(1.f, e);
  }
  scale[0] = s;
  scale[1] = 1.f / s;
  *amax_bits = 0u;  // (re-armed for the next call)
}

}  // namespace tcavt

using namespace tcavt;

extern "C" int tcavt_silu_mul_bwd(const void* gu_bf16, const void* g_act_bf16, void* g_gu_bf16, int64_t M, int I, int dtype16,
                                  tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(is16(dtype16), "silu_mul_bwd: dtype16 must be TCAVT_BF16 or TCAVT_F16");
  TCAVT_CHECK_ARG(gu_bf16 && g_act_bf16 && g_gu_bf16 && M > 0 && I > 0 && I % 16 == 0, "silu_mul_bwd: bad args (I %% 16 == 0)");
  TCAVT_CHECK_ARG(aligned16(gu_bf16) && aligned16(g_act_bf16) && aligned16(g_gu_bf16), "silu_mul_bwd: 16-byte alignment required");
  const long n = (long)M * (I / 16);
  auto kfn = dtype16 == TCAVT_F16 ? silu_mul_bwd_kernel<true> : silu_mul_bwd_kernel<false>;
  hipLaunchKernelGGL(kfn, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(gu_bf16), static_cast<const bf16_t*>(g_act_bf16),
                     static_cast<bf16_t*>(g_gu_bf16), (long)M, I);
  TCAVT_CHECK_LAUNCH("silu_mul_bwd");
  return TCAVT_OK;
}

extern "C" int tcavt_rmsnorm_bwd(const void* x, const float* gamma, const void* gy_bf16, const void* gy2_bf16, float eps,
                                 float* gx, void* gx_bf16, int accumulate, int M, int H, int gy_dtype, int out_dtype,
                                 const float* gy_scale, int x_dtype, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(is16(gy_dtype) && (gx_bf16 == nullptr || is16(out_dtype)), "rmsnorm_bwd: gy_dtype / out_dtype must be TCAVT_BF16 or TCAVT_F16");
  TCAVT_CHECK_ARG(x_dtype == TCAVT_F32 || is16(x_dtype), "rmsnorm_bwd: x_dtype must be TCAVT_F32, TCAVT_F16 or TCAVT_BF16");
  TCAVT_CHECK_ARG(x && gamma && gy_bf16 && gx && M > 0 && H > 0 && H % 8 == 0, "rmsnorm_bwd: bad args (H %% 8 == 0)");
  TCAVT_CHECK_ARG(aligned16(x) && aligned16(gamma) && aligned16(gy_bf16) && aligned16(gy2_bf16) && aligned16(gx) &&
                      aligned16(gx_bf16), "rmsnorm_bwd: 16-byte alignment required");
  typedef decltype(&rmsnorm_bwd_kernel<false, false, 0>) kfn_t;
  static const kfn_t kfns[3][2][2] = {  // [XT][GF16][OF16]
      {{rmsnorm_bwd_kernel<false, false, 0>, rmsnorm_bwd_kernel<false, true, 0>}, {rmsnorm_bwd_kernel<true, false, 0>, rmsnorm_bwd_kernel<true, true, 0>}},
      {{rmsnorm_bwd_kernel<false, false, 1>, rmsnorm_bwd_kernel<false, true, 1>}, {rmsnorm_bwd_kernel<true, false, 1>, rmsnorm_bwd_kernel<true, true, 1>}},
      {{rmsnorm_bwd_kernel<false, false, 2>, rmsnorm_bwd_kernel<false, true, 2>}, {rmsnorm_bwd_kernel<true, false, 2>, rmsnorm_bwd_kernel<true, true, 2>}}};
  const kfn_t kfn = kfns[x_dtype == TCAVT_F32 ? 0 : x_dtype == TCAVT_F16 ? 1 : 2][gy_dtype == TCAVT_F16][out_dtype == TCAVT_F16];
  hipLaunchKernelGGL(kfn, dim3((M + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), x, gamma,
                     static_cast<const bf16_t*>(gy_bf16), static_cast<const bf16_t*>(gy2_bf16), eps, gx,
                     static_cast<bf16_t*>(gx_bf16), accumulate, M, H, gy_scale);
  TCAVT_CHECK_LAUNCH("rmsnorm_bwd");
  return TCAVT_OK;
}

#define TCAVT_TRY(call)            \
  do {                             \
    const int rc_ = (call);        \
    if (rc_ != TCAVT_OK) return rc_; \
  } while (0)

extern "C" int tcavt_llama_stack_backward(const tcavt_llama_backward_args* a, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(a && a->layers && a->h_last && a->gamma_final && a->g_final_a && a->rope_cos && a->rope_sin && a->kv_len && a->scale &&
                      a->scale_scratch && a->g_h && a->g_hb && a->g_xn && a->g_xl && a->g_att && a->g_qkv0 && a->g_qkv1 && a->g_t0 &&
                      a->g_t1 && a->dA && a->dB && a->stats,
                  "llama_stack_backward: null pointer");
  const int B = a->B, L = a->L, H = a->H, I = a->I, nq = a->nq, nkv = a->nkv, dt = a->dtype16, r = a->lora_rank;
  TCAVT_CHECK_ARG(a->n_layers > 0 && B > 0 && L > 0 && is16(dt) && nkv > 0 && nq % nkv == 0 && r > 0 && r <= 16 && a->npart > 0,
                  "llama_stack_backward: bad shape");
  // fp16 tapes only: the 16-bit residual-stream tapes this walk reads exist for fp16 storage alone (bf16 storage keeps fp32
  // streams, whose backward is the per-launch composition of llm_backward.py); head_dim 64, adapters in 16-column groups
  TCAVT_CHECK_ARG(dt == TCAVT_F16, "llama_stack_backward: dtype16 must be TCAVT_F16 (16-bit stream tapes exist for fp16 storage only)");
  const int M = B * L, nqkv = (nq + 2 * nkv) * 64;
  // L <= 256: resident; 256 < L <= 544: chunked (tcavt_attn_bwd_long); 544 < L <= 2048: chunked (tcavt_attn_bwd_stream)
  decltype(&tcavt_attn_bwd_resident) attn_bwd = tcavt_attn_bwd_resident_ok(L, nq, nkv) ? tcavt_attn_bwd_resident
                                                : tcavt_attn_bwd_long_ok(L, nq, nkv)   ? tcavt_attn_bwd_long
                                                : tcavt_attn_bwd_stream_ok(L, nq, nkv) ? tcavt_attn_bwd_stream
                                                                                       : nullptr;
  TCAVT_CHECK_ARG(attn_bwd && M % 256 == 0 && I % 256 == 0 && H % 128 == 0,
                  "llama_stack_backward: outside the fused forms (L <= 2048, 16 %% (nq / nkv) == 0, M %% 256 == 0, I %% 256 == 0, H %% 128 == 0)");
  TCAVT_CHECK_ARG(!a->leaf_stream || a->events, "llama_stack_backward: a leaf stream needs the four events");
  // every layer's pointers are checked BEFORE anything is launched: an argument error must not leave half a walk enqueued
  // (adapter gradients half-written, the leaf stream forked and never joined -- under a hipGraph capture an unjoined stream)
  for (int li = 0; li < a->n_layers; ++li) {
    const tcavt_llama_bwd_layer& w = a->layers[li];
    TCAVT_CHECK_ARG(w.w_dT && w.w_guT && w.w_oT && w.w_qkvT && w.b_extT && w.a_qT && w.a_vT && w.g1 && w.g2 && w.h_in && w.h_mid && w.qkv &&
                        w.gu && w.att && w.lse && w.part && w.t && w.g_Aq && w.g_Av && w.g_Bq && w.g_Bv,
                    "llama_stack_backward: layer %d: null pointer", li);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipStream_t lf = a->leaf_stream ? static_cast<hipStream_t>(a->leaf_stream) : st;
  const bool two = lf != st;
  const bool f16 = dt == TCAVT_F16;
  const int gdt = f16 ? TCAVT_BF16 : dt;  // type of the incoming gradients
  if (f16) TCAVT_TRY(tcavt_grad_scale_pick(a->g_final_a, a->g_final_b, (int64_t)M * H, TCAVT_BF16, 256.f, a->scale, a->scale_scratch,
                                           a->scale_backoff, stream));
  const float* inv_s = a->scale + 1;
  // final norm: g_h = d(rmsnorm)(h_last) . (g_final_a + g_final_b) * S,  g_hb = its 16-bit copy
  TCAVT_TRY(tcavt_rmsnorm_bwd(a->h_last, a->gamma_final, a->g_final_a, a->g_final_b, a->rms_eps, a->g_h, a->g_hb, 0, M, H, gdt, dt,
                              f16 ? a->scale : nullptr, dt, stream));
  auto gemm = [&](const void* A, int lda, const void* W, int K, void* C, int N, float acc_scale) -> int {
    tcavt_gemm_args g = {};
    g.A = A; g.lda = lda; g.W = W; g.ldw = K; g.C = C; g.ldc = N; g.M = M; g.N = N; g.K = K;
    g.out_dtype = dt; g.in_dtype = dt; g.acc_scale = acc_scale;
    return tcavt_gemm_bf16(&g, stream);
  };
  auto hip_ok = [&](hipError_t rc, const char* what) -> int {
    if (rc == hipSuccess) return TCAVT_OK;
    set_error("llama_stack_backward: %s: %s", what, hipGetErrorString(rc));
    return TCAVT_ERR_HIP;
  };
  bool leaf_used[2] = {false, false};
  bool scratch_zeroed = false;
  void* const g_qkv2[2] = {a->g_qkv0, a->g_qkv1};
  void* const g_t2[2] = {a->g_t0, a->g_t1};
  // (the walk is a lambda so that a failure in the middle of it -- a launch error; the arguments were checked above -- still
  //  reaches the join below: the caller's stream then waits for whatever the leaf stream was given)
  auto walk = [&]() -> int {
  for (int li = a->n_layers - 1; li >= 0; --li) {
    const tcavt_llama_bwd_layer& w = a->layers[li];
    // ---- MLP half
    {
      tcavt_gemm_args g = {};
      g.A = a->g_hb; g.lda = H; g.W = w.w_dT; g.ldw = H; g.C = w.gu; g.ldc = 2 * I; g.M = M; g.N = I; g.K = H;
      g.out_dtype = dt; g.in_dtype = dt; g.silu_preact = w.gu; g.ld_preact = 2 * I; g.epilogue = TCAVT_EPI_SILU_BWD;
      TCAVT_TRY(tcavt_gemm_bf16(&g, stream));
    }
    TCAVT_TRY(gemm(w.gu, 2 * I, w.w_guT, 2 * I, a->g_xn, H, 0.f));
    TCAVT_TRY(tcavt_rmsnorm_bwd(w.h_mid, w.g2, a->g_xn, nullptr, a->rms_eps, a->g_h, a->g_hb, 1, M, H, dt, dt, nullptr, dt, stream));
    // ---- attention half
    TCAVT_TRY(gemm(a->g_hb, H, w.w_oT, H, a->g_att, nq * 64, 0.f));
    const int par = li & 1;
    if (two && leaf_used[par])  // the leaf of layer li + 2 has read g_qkv / g_t of this parity
      TCAVT_TRY(hip_ok(hipStreamWaitEvent(st, static_cast<hipEvent_t>(a->events[2 + par]), 0), "wait(done)"));
    TCAVT_TRY(attn_bwd(w.qkv, a->g_att, w.att, w.lse, g_qkv2[par], a->stats, a->rope_cos, a->rope_sin, a->kv_len, B, L, nq, nkv, 64, 0.125f,
                       dt, stream));
    TCAVT_TRY(gemm(g_qkv2[par], nqkv, w.b_extT, nqkv, g_t2[par], 64, a->lora_scale));
    // ---- leaf: the adapters' weight gradients (nothing downstream reads them)
    if (two) {
      TCAVT_TRY(hip_ok(hipEventRecord(static_cast<hipEvent_t>(a->events[par]), st), "record(ready)"));
      TCAVT_TRY(hip_ok(hipStreamWaitEvent(lf, static_cast<hipEvent_t>(a->events[par]), 0), "wait(ready)"));
    }
    {
      const uint32_t site = a->lora_first_site + 2u * (uint32_t)li;
      if (!scratch_zeroed) {  // (once per walk: adapter_grads_out_kernel leaves the scratch zero for the next layer)
        TCAVT_TRY(hip_ok(hipMemsetAsync(a->dA, 0, (size_t)64 * H * sizeof(float), lf), "memset(dA)"));
        TCAVT_TRY(hip_ok(hipMemsetAsync(a->dB, 0, (size_t)nqkv * 64 * sizeof(float), lf), "memset(dB)"));
        scratch_zeroed = true;
      }
      TCAVT_TRY(tcavt_lora_wgrad_a(w.h_in, w.part, a->npart, a->rms_eps, w.g1, g_t2[par], a->dA, H, M, H, a->lora_dropout_p,
                                   a->dropout_seed, site, site + 1, dt, lf));
      TCAVT_TRY(tcavt_wgrad_tn(w.t, 64, 0, 32, g_qkv2[par], nqkv, dt, a->dB, 64, M, nqkv, 1, dt, w.part, a->npart, H, a->rms_eps, lf));
      const long n_out = (long)64 * H + (long)nqkv * 64;
      hipLaunchKernelGGL(adapter_grads_out_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, lf, a->dA, a->dB, w.g_Aq, w.g_Av,
                         w.g_Bq, w.g_Bv, H, nqkv, nq * 64, (nq + nkv) * 64, r, f16 ? inv_s : nullptr);
      TCAVT_CHECK_LAUNCH("llama_stack_backward(adapter gradients)");
    }
    if (two) {
      TCAVT_TRY(hip_ok(hipEventRecord(static_cast<hipEvent_t>(a->events[2 + par]), lf), "record(done)"));
      leaf_used[par] = true;
    }
    if (li == 0 && !a->input_grad) break;
    {
      const uint32_t site = a->lora_first_site + 2u * (uint32_t)li;
      TCAVT_TRY(tcavt_lora_dgrad(g_t2[par], w.a_qT, w.a_vT, a->g_xl, M, H, a->lora_dropout_p, a->dropout_seed, site, site + 1, dt, stream));
    }
    TCAVT_TRY(gemm(g_qkv2[par], nqkv, w.w_qkvT, nqkv, a->g_xn, H, 0.f));
    TCAVT_TRY(tcavt_rmsnorm_bwd(w.h_in, w.g1, a->g_xn, a->g_xl, a->rms_eps, a->g_h, a->g_hb, 1, M, H, dt, dt, nullptr, dt, stream));
  }
  return TCAVT_OK;
  };
  const int rc_walk = walk();
  int rc_join = TCAVT_OK;
  if (two) {
    if (rc_walk != TCAVT_OK) {
      // the failing layer may have forked the leaf stream without recording its `done` event: one more record covers
      // everything that stream was given, and the join below waits for it
      if (hipEventRecord(static_cast<hipEvent_t>(a->events[2]), lf) == hipSuccess) leaf_used[0] = true;
    }
    for (int par = 0; par < 2; ++par)
      if (leaf_used[par] && hipStreamWaitEvent(st, static_cast<hipEvent_t>(a->events[2 + par]), 0) != hipSuccess && rc_walk == TCAVT_OK) {
        set_error("llama_stack_backward: join(leaf) failed");
        rc_join = TCAVT_ERR_HIP;
      }
  }
  return rc_walk != TCAVT_OK ? rc_walk : rc_join;
}

extern "C" int tcavt_clip_grad_norm(float* g, int64_t n, float max_norm, float grad_scale, float* scratch,
                                    tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(g && scratch && n > 0 && max_norm > 0.f && grad_scale > 0.f, "clip_grad_norm: bad args");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(CLIP_BLOCKS), dim3(256), 0, st, g, (long)n, scratch);
  hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(64), 0, st, scratch, max_norm, grad_scale);
  long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(scale_by_kernel, dim3((unsigned)blocks), dim3(256), 0, st, g, (long)n, scratch + CLIP_BLOCKS);
  TCAVT_CHECK_LAUNCH("clip_grad_norm");
  return TCAVT_OK;
}

// Grid of wgrad_tn_kernel and lora_wgrad_a_kernel over an [M, H] operand: gx blocks of 256 columns, times `split` ranges
// of m_per_wg rows (a multiple of the 32 rows of one step)
struct RowSplit {
  int gx, split, m_per_wg;
};
static RowSplit row_split(int M, int H) {
  const int gx = (H + 255) / 256;
  int split = 256 / gx;  // ~one workgroup per CU
  if (split < 1) split = 1;
  const int m_per_wg = ((M + split - 1) / split + 31) / 32 * 32;
  return {gx, (M + m_per_wg - 1) / m_per_wg, m_per_wg};
}

extern "C" int tcavt_wgrad_tn(const void* G, int64_t ldg, int g_col0, int n, const void* X, int64_t ldx, int x_dtype, float* C,
                              int64_t ldc, int M, int H, int trans_out, int g_dtype, const float* rs_part, int rs_npart, int rs_h,
                              float rs_eps, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(!rs_part || (rs_npart > 0 && rs_npart % 4 == 0 && rs_h > 0 && aligned16(rs_part)),
                  "wgrad_tn: rs_part needs rs_npart %% 4 == 0, rs_h > 0 and 16-byte alignment");
  const float rs_inv_h = rs_part ? 1.f / (float)rs_h : 0.f;
  TCAVT_CHECK_ARG(G && X && C && M > 0 && H > 0 && n > 0 && n <= 64 && n % 16 == 0 && g_col0 >= 0 && g_col0 % 8 == 0 &&
                      ldg % 8 == 0 && ldx % 8 == 0 && H % 8 == 0 && is16(x_dtype),
                  "wgrad_tn: n in {16, 32, 48, 64}, g_col0 / ldg / ldx / H multiples of 8");
  TCAVT_CHECK_ARG(g_dtype == 0 || g_dtype == TCAVT_BF16 || (g_dtype == TCAVT_F16 && x_dtype == TCAVT_F16),
                  "wgrad_tn: G is bf16 (g_dtype 0 / TCAVT_BF16), or fp16 together with an fp16 X");
  TCAVT_CHECK_ARG(aligned16(G) && aligned16(X), "wgrad_tn: 16-byte alignment required");
  const RowSplit s = row_split(M, H);
  auto kfn = g_dtype == TCAVT_F16 ? wgrad_tn_kernel<true, true> : x_dtype == TCAVT_F16 ? wgrad_tn_kernel<true> : wgrad_tn_kernel<false>;
  hipLaunchKernelGGL(kfn, dim3(s.gx, s.split), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(G),
                     (long)ldg, g_col0, n / 16, static_cast<const bf16_t*>(X), (long)ldx, C, (long)ldc, M, H, s.m_per_wg, trans_out,
                     rs_part, rs_npart, rs_inv_h, rs_eps);
  TCAVT_CHECK_LAUNCH("wgrad_tn");
  return TCAVT_OK;
}

extern "C" int tcavt_lora_wgrad_a(const void* x16, const float* part, int npart, float eps, const float* gamma, const void* g_t,
                                  float* dA, int64_t ldc, int M, int H, float dropout_p, uint64_t dropout_seed, uint32_t site_q,
                                  uint32_t site_v, int dtype16, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(x16 && part && gamma && g_t && dA && M > 0 && H > 0 && H % 16 == 0 && npart > 0 && npart % 4 == 0 && ldc >= H &&
                      is16(dtype16) && dropout_p >= 0.f && dropout_p < 1.f,
                  "lora_wgrad_a: bad args (H %% 16 == 0, npart %% 4 == 0, ldc >= H, 0 <= dropout_p < 1)");
  TCAVT_CHECK_ARG(aligned16(x16) && aligned16(part) && aligned16(g_t), "lora_wgrad_a: 16-byte alignment required");
  const DropoutP dq = make_dropout(dropout_p, dropout_seed, site_q), dv = make_dropout(dropout_p, dropout_seed, site_v);
  const RowSplit s = row_split(M, H);
  auto kfn = dtype16 == TCAVT_F16 ? lora_wgrad_a_kernel<true> : lora_wgrad_a_kernel<false>;
  hipLaunchKernelGGL(kfn, dim3(s.gx, s.split), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(x16), part, npart,
                     1.f / (float)H, eps, gamma, static_cast<const bf16_t*>(g_t), dA, (long)ldc, M, H, s.m_per_wg, dq, dv);
  TCAVT_CHECK_LAUNCH("lora_wgrad_a");
  return TCAVT_OK;
}

extern "C" int tcavt_grad_scale_pick(const void* g_a, const void* g_b, int64_t n, int dtype16, float target, float* scale,
                                     uint32_t* scratch, const int32_t* backoff, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(g_a && scale && scratch && n > 0 && n % 8 == 0 && is16(dtype16) && target > 0.f && aligned16(g_a) && aligned16(g_b),
                  "grad_scale_pick: bad args (n %% 8 == 0, 16-byte alignment, scratch = one zero-initialised uint32)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  long blocks = (n / 8 + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  auto kfn = dtype16 == TCAVT_F16 ? grad_amax_kernel<true> : grad_amax_kernel<false>;
  hipLaunchKernelGGL(kfn, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const bf16_t*>(g_a), static_cast<const bf16_t*>(g_b),
                     (long)(n / 8), scratch);
  hipLaunchKernelGGL(grad_scale_set_kernel, dim3(1), dim3(1), 0, st, scratch, target, scale, backoff);
  TCAVT_CHECK_LAUNCH("grad_scale_pick");
  return TCAVT_OK;
}
