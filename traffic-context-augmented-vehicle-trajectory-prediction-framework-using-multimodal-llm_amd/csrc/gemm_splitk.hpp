// Helper kernels around the GEMM: the fragment-major weight copy of the skinny form and the reduce step of the
// two-launch split-K form of the in-place 16-bit residual GEMM.
#pragma once
#include "gemm_params.hpp"

namespace tcavt {

// ---------------------------------------------------------------------------
// Fragment-major copy of a weight matrix for the skinny form (tcavt.h: tcavt_pack_weight16).  One thread per 16-byte piece:
// piece (b, j, l) <- W[16 b + (l & 15)][32 j + 8 (l >> 4) .. + 7]; the writes are consecutive, the reads 16 rows x 64 bytes.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_weight16_kernel(const bf16_t* __restrict__ W, long ldw, bf16_t* __restrict__ out, int N, int K) {
  const long piece = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)N * K / 8;
  if (piece >= total) return;
  const int l = (int)(piece & 63);
  const long chunk = piece >> 6;
  const int ksteps = K >> 5;
  const long b = chunk / ksteps;
  const int j = (int)(chunk - b * ksteps);
  const u32x4 v = *reinterpret_cast<const u32x4*>(W + (16 * b + (l & 15)) * ldw + 32 * j + 8 * (l >> 4));
  *reinterpret_cast<u32x4*>(out + piece * 8) = v;
}

// ---------------------------------------------------------------------------
// FP8 copy of a weight matrix for the skinny form (tcavt.h: tcavt_pack_weight8): OCP e4m3fn codes in the fragment-major order
// above at one byte per element, one power-of-two scale per row behind them.
// ---------------------------------------------------------------------------
// (e4m3_code / e4m3_row_exp: common.hpp)
// One workgroup per block of 16 rows; 16 consecutive lanes per row find its largest magnitude (and whether all of it is finite),
// then thread t writes the 8-byte pieces t, t + 256, ... of the block's K / 32 chunks: piece (j, l) <- W[16 b + (l & 15)][32 j +
// 8 (l >> 4) .. + 7] * 2^-k (exact: ldexp), rounded once.  A row with a non-finite element: the NaN code everywhere, scale 1.
template <bool F16>
__global__ __launch_bounds__(256) void pack_weight8_kernel(const bf16_t* __restrict__ W, long ldw, unsigned char* __restrict__ out, int N, int K) {
  __shared__ int row_k[16];
  __shared__ int row_bad[16];
  const long b = blockIdx.x;
  const int t = threadIdx.x, r = t >> 4, part = t & 15;
  const bf16_t* row = W + (16 * b + r) * ldw;
  unsigned int amax_bits = 0u;  // (non-negative floats order like their bit patterns; inf / NaN end up on top)
  for (int c = part * 8; c < K; c += 128) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(row + c);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      amax_bits = max(amax_bits, __builtin_bit_cast(unsigned int, from16_lo<F16>(v[i])) & 0x7fffffffu);
      amax_bits = max(amax_bits, __builtin_bit_cast(unsigned int, from16_hi<F16>(v[i])) & 0x7fffffffu);
    }
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) amax_bits = max(amax_bits, (unsigned int)__shfl_xor((int)amax_bits, o, 64));
  if (part == 0) {
    const bool bad = amax_bits >= 0x7f800000u;
    const int k = (bad || amax_bits == 0u) ? 0 : e4m3_row_exp(__builtin_bit_cast(float, amax_bits));
    row_k[r] = k;
    row_bad[r] = bad;
    reinterpret_cast<float*>(out + (long)N * K)[16 * b + r] = ldexpf(1.f, k);
  }
  __syncthreads();
  const int pieces = (K >> 5) * 64;
  unsigned char* dst = out + b * 16 * K;
  for (int pc = t; pc < pieces; pc += 256) {
    const int l = pc & 63, j = pc >> 6, rr = l & 15;
    const u32x4 v = *reinterpret_cast<const u32x4*>(W + (16 * b + rr) * ldw + 32 * j + 8 * (l >> 4));
    const int k = row_k[rr];
    u32x2 o = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned int lo = e4m3_code(ldexpf(from16_lo<F16>(v[i]), -k)), hi = e4m3_code(ldexpf(from16_hi<F16>(v[i]), -k));
      o[i >> 1] |= (lo | (hi << 8)) << (16 * (i & 1));
    }
    if (row_bad[rr]) o = u32x2{0x7f7f7f7fu, 0x7f7f7f7fu};
    *reinterpret_cast<u32x2*>(dst + (long)pc * 8) = o;
  }
}

// ---------------------------------------------------------------------------
// Split K for residual GEMMs that cannot fill the chip (round 4).  At M = 1024 (BASELINE config 4's low end: B = 8, L = 128) the
// o / down projections are 128 tiles of 128 x 128 -- half the CUs, one 4-wave workgroup each walking 32 / 128 K-tiles alone at
// ~1 us per K-tile (its waves issue DMA, fragment loads and MFMAs one after the other; nothing else is resident to overlap
// them): 30 / 90 us where the arithmetic is worth 7 / 29.  With a workspace the launch becomes TWO: (1) the S partial products
// over K / S as a batched launch of the generic fp32 form into S slabs [M][N] -- 4 x the workgroups, two per CU on the 64 KiB
// form, each a quarter of the chain -- and (2) this kernel: slabs added in slice order (bit-reproducible), then exactly the
// in-place 16-bit residual epilogue of TCAVT_EPI_NORM_OUT (round(norm_scale * acc + h16), partial sums of squares of the rounded
// values per 64 columns, range flag).  No cross-workgroup hand-off inside a kernel: the launch boundary is the reduction's barrier.
// ---------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(256) void splitk_norm16_kernel(const float* __restrict__ slabs, int S, long slab_stride,
                                                            const bf16_t* __restrict__ res16, bf16_t* __restrict__ out16,
                                                            float* __restrict__ part, int M, int N, long ldc, int npart, float nscale,
                                                            int has_res, int* __restrict__ nf_flag, int nf_tag) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;  // one thread: 8 consecutive columns of one row
  const int per_row = N >> 3;
  const long m = idx / per_row;
  const int c0 = (int)(idx - m * per_row) * 8;
  const bool on = m < M;
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
  u32x4 old = {0u, 0u, 0u, 0u};
  if (on) {
    const float* sp = slabs + m * N + c0;
    if (has_res) old = *reinterpret_cast<const u32x4*>(res16 + m * ldc + c0);
    for (int s_ = 0; s_ < S; ++s_) {  // (slice order: the sum does not depend on which workgroup finished first)
      a0 += *reinterpret_cast<const f32x4*>(sp + s_ * slab_stride);
      a1 += *reinterpret_cast<const f32x4*>(sp + s_ * slab_stride + 4);
    }
  }
  const f32x4 v0 = fma4(a0, nscale, f32x4{from16_lo<F16>(old[0]), from16_hi<F16>(old[0]), from16_lo<F16>(old[1]), from16_hi<F16>(old[1])});
  const f32x4 v1 = fma4(a1, nscale, f32x4{from16_lo<F16>(old[2]), from16_hi<F16>(old[2]), from16_lo<F16>(old[3]), from16_hi<F16>(old[3])});
  const u32x4 w = {pack16x2<F16>(v0[0], v0[1]), pack16x2<F16>(v0[2], v0[3]), pack16x2<F16>(v1[0], v1[1]), pack16x2<F16>(v1[2], v1[3])};
  float ss = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float lo = from16_lo<F16>(w[e]), hi = from16_hi<F16>(w[e]);
    ss += lo * lo;
    ss += hi * hi;
  }
  if (on) *reinterpret_cast<u32x4*>(out16 + m * ldc + c0) = w;
  if (!on) ss = 0.f;
  ss += __shfl_xor(ss, 1, 64);  // the 8 lanes of a 64-column group are consecutive (N % 64 == 0)
  ss += __shfl_xor(ss, 2, 64);
  ss += __shfl_xor(ss, 4, 64);
  if (on && (threadIdx.x & 7) == 0) {
    part[m * npart + (c0 >> 6)] = ss;
    if (nf_flag && !(ss <= 3.0e38f)) atomicCAS(nf_flag, 0, nf_tag);
  }
}

// slices for the two-launch split: enough 128 x 128 tiles for ~two workgroups per CU, slices of whole K-tiles and >= 2048 deep --
// measured at M = 1024 (one box, in the model): down (K = 8192) 87.6 -> 53.7 us with S = 4; o (K = 2048) 29.8 -> 29.7 with S = 4
// and 31.4 -> 40.0 at M = 2048 with S = 2: a 512-deep slice is all pipeline fill, and the reduce kernel costs what the split saves
static int splitk_slices(int M, int N, int K) {
  const long wg = (long)((M + 127) / 128) * (N / 128);
  int S = 1;
  while (S < 8 && wg * S * 2 <= 512 && K % (S * 2 * 64) == 0 && K / (S * 2) >= 2048) S *= 2;
  return S;
}

}  // namespace tcavt
