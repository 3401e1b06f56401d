// The 8-wave (and 2 x 2-wave small-tile) GEMM kernel: tile codes 64, 128 and 256.  The staging scheme, the LDS image and
// the swapped MFMA operand order are described at the top of gemm_bf16.hip.
#pragma once
#include "gemm_epilogue.hpp"

namespace tcavt {

template <int BM, int BN, int WARPS_M, int WARPS_N, int EPI, bool F16, int PIPE>
__global__ __launch_bounds__(WARPS_M* WARPS_N * 64) void gemm_bf16_kernel(GemmP p) {
  constexpr int NW = WARPS_M * WARPS_N;
  constexpr int ROWS = BM + BN;
  constexpr int TILE_BYTES = ROWS * 128;
  constexpr int WTM = BM / WARPS_M, WTN = BN / WARPS_N;
  constexpr int TM = WTM / 16, TN = WTN / 16;
  constexpr int ROUNDS = ROWS / (8 * NW);
  static_assert(ROWS % (8 * NW) == 0, "staging rounds must be whole");
  static_assert(BM % 16 == 0 && BN % 16 == 0, "tile rows");
  static_assert(EPI != EPI_ROPE || WTN % 64 == 0, "RoPE needs whole heads per wave");
  static_assert((EPI != EPI_SILU && EPI != EPI_SILU_SAVE) || WTN % 32 == 0, "SiLU needs gate/up pairs per wave");
  static_assert(PIPE == 1 || PIPE == 2, "main loop: 1 = two LDS stages, DMA pieces between the MFMAs; 2 = four LDS stages");

  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / WARPS_N, wn = wave % WARPS_N;

  // ---- block -> tile (XCD-aware; any bijection is correct, this one is for L2 / fabric traffic)
  int tile_m, tile_n;
  block_to_tile(p, tile_m, tile_n);
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  if (gridDim.y > 1) {  // batched form: product blockIdx.y
    const int bo = blockIdx.y / p.batch_inner, bi = blockIdx.y - bo * p.batch_inner;
    p.A += bo * p.sAo + bi * p.sAi;
    p.W += bo * p.sWo + (bi / p.w_group) * p.sWi;
    const long co = bo * p.sCo + bi * p.sCi;
    p.C = p.out_kind == TCAVT_F32 ? static_cast<void*>(reinterpret_cast<float*>(p.C) + co)
                                  : static_cast<void*>(reinterpret_cast<bf16_t*>(p.C) + co);
  }

  // ---- per-lane staging sources (main K source), one per round
  const bf16_t* src[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int g = r * NW + wave;
    const int row = g * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((row >> 1) & 7);
    if (g * 8 < BM) {
      const int m = min(m0 + row, p.M - 1);
      src[r] = p.A + (long)m * p.lda + c * 8;
    } else {
      const int n = min(n0 + row - BM, p.N - 1);
      src[r] = p.W + (long)n * p.ldw + c * 8;
    }
  }
  const int nt1 = p.K >> 6, nt = nt1 + (p.K2 >> 6);

  auto stage = [&](int buf, int t) {
    char* base = smem + buf * TILE_BYTES;
    if (t < nt1) {
#pragma unroll
      for (int r = 0; r < ROUNDS; ++r) glds16(src[r] + t * 64, base + (r * NW + wave) * 1024);
    } else {
      const int k0 = (t - nt1) * 64;
#pragma unroll
      for (int r = 0; r < ROUNDS; ++r) {
        const int g = r * NW + wave;
        const int row = g * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((row >> 1) & 7);
        const bf16_t* s;
        if (g * 8 < BM) {
          const int m = min(m0 + row, p.M - 1);
          s = p.A2 + (long)m * p.lda2 + k0 + c * 8;
        } else {
          const int n = min(n0 + row - BM, p.N - 1);
          s = p.W2 + (long)n * p.ldw2 + k0 + c * 8;
        }
        glds16(s, base + g * 1024);
      }
    }
  };

  // ---- fragment read addressing
  const int fsw = (lane >> 1) & 7;  // == (row>>1)&7 for row = 16*j + (lane&15)
  const int off0 = (((lane >> 4)) ^ fsw) * 16;
  const int off1 = ((4 + (lane >> 4)) ^ fsw) * 16;
  const int xrow = (wm * WTM + (lane & 15)) * 128;
  const int wrow = (BM + wn * WTN + (lane & 15)) * 128;

  f32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int buf) {
    const char* base = smem + buf * TILE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int off = ks ? off1 : off0;
      bf16x8 wf[TN], xf[TM];
#pragma unroll
      for (int i = 0; i < TN; ++i)
        wf[i] = *reinterpret_cast<const bf16x8*>(base + wrow + i * 2048 + off);
#pragma unroll
      for (int j = 0; j < TM; ++j)
        xf[j] = *reinterpret_cast<const bf16x8*>(base + xrow + j * 2048 + off);
      if (p.prio == 2) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j)
          if constexpr (F16)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, wf[i]),
                                                               __builtin_bit_cast(f16x8, xf[j]), acc[i][j], 0, 0, 0);
          else
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], xf[j], acc[i][j], 0, 0, 0);
      if (p.prio == 2) __builtin_amdgcn_s_setprio(0);
    }
  };

  // PIPE == 1: the DMA pieces of tile t+1 are issued one at a time BETWEEN the MFMAs of the
  // first k-step of tile t instead of in one burst ahead of them (each piece costs the issuing wave
  // ~60-180 cycles of issue time; spread out, the other wave of the SIMD keeps the matrix pipe busy).
  auto compute_interleaved = [&](int buf, int nbuf, int tn) {
    const char* base = smem + buf * TILE_BYTES;
    char* nbase = smem + nbuf * TILE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int off = ks ? off1 : off0;
      bf16x8 wf[TN], xf[TM];
#pragma unroll
      for (int i = 0; i < TN; ++i) wf[i] = *reinterpret_cast<const bf16x8*>(base + wrow + i * 2048 + off);
#pragma unroll
      for (int j = 0; j < TM; ++j) xf[j] = *reinterpret_cast<const bf16x8*>(base + xrow + j * 2048 + off);
      if (p.prio == 2) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) {
          if constexpr (F16)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, wf[i]),
                                                               __builtin_bit_cast(f16x8, xf[j]), acc[i][j], 0, 0, 0);
          else
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], xf[j], acc[i][j], 0, 0, 0);
          constexpr int PER = (TN * TM) / ROUNDS;  // MFMAs per DMA piece
          const int idx = i * TM + j;
          if (ks == 0 && (idx % PER) == PER - 1) {
            const int r = idx / PER;
            glds16(src[r] + tn * 64, nbase + (r * NW + wave) * 1024);
          }
        }
      if (p.prio == 2) __builtin_amdgcn_s_setprio(0);
    }
  };

  if constexpr (PIPE == 2) {
    // ---- deep main loop for launches that cannot fill the chip (a few dozen workgroups, each walking its K
    // range alone): four LDS stages, up to three K-tiles of DMA in flight, so that a K-tile costs its issue
    // time instead of a full HBM / L2 round trip (the weights of these layers are HBM-cold inside the model).
    // Counted vmcnt (the wave's own pieces of the NEWER tiles stay in flight) and a raw barrier per K-tile:
    // the barrier publishes tile t and proves everyone is done with tile t-1, whose stage the next DMA reuses.
    constexpr int NS = 4;
#pragma unroll
    for (int s = 0; s < NS - 1; ++s)
      if (s < nt) stage(s, s);
    for (int t = 0; t < nt; ++t) {
      const int rem = nt - 1 - t;
      if (rem >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * ROUNDS) : "memory");
      else if (rem == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(ROUNDS) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_barrier" ::: "memory");
      if (t + NS - 1 < nt) stage((t + NS - 1) % NS, t + NS - 1);
      compute(t % NS);
    }
    gemm_epilogue<TM, TN, EPI, false, F16>(p, acc, m0 + wm * WTM, n0 + wn * WTN, lane);
    return;
  }
  if (p.prio == 1 && wave >= NW / 2) __builtin_amdgcn_s_setprio(1);
  // ---- main loop: stage t+1 while computing t; one drain+barrier per K-tile
  stage(0, 0);
  __syncthreads();
  int cur = 0;
  int t = 0;
  for (; t + 1 < nt1; ++t) {
    compute_interleaved(cur, cur ^ 1, t + 1);
    __syncthreads();
    cur ^= 1;
  }
  for (; t < nt - 1; ++t) {  // second K-source (LoRA): burst staging
    stage(cur ^ 1, t + 1);
    compute(cur);
    __syncthreads();
    cur ^= 1;
  }
  compute(cur);

  gemm_epilogue<TM, TN, EPI, false, F16>(p, acc, m0 + wm * WTM, n0 + wn * WTN, lane);
}

template <int BM, int BN, int WARPS_M, int WARPS_N, int EPI, bool F16, int PIPE>
static int launch(const GemmP& p0, int batch, hipStream_t stream) {
  GemmP p = p0;
  p.tiles_m = (p.M + BM - 1) / BM;
  p.tiles_n = (p.N + BN - 1) / BN;
  p.xcd_gx = choose_xcd_partition(p);
  constexpr int lds = (PIPE == 2 ? 4 : 2) * (BM + BN) * 128;
  auto kfn = gemm_bf16_kernel<BM, BN, WARPS_M, WARPS_N, EPI, F16, PIPE>;
  static bool attr_set = false;  // per instantiation
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) {
      set_error("gemm_bf16: hipFuncSetAttribute(%d B LDS) failed: %s", lds, hipGetErrorString(e));
      return TCAVT_ERR_HIP;
    }
    attr_set = true;
  }
  dim3 grid(p.tiles_m * p.tiles_n, batch), block(WARPS_M * WARPS_N * 64);
  hipLaunchKernelGGL(kfn, grid, block, lds, stream, p);
  TCAVT_CHECK_LAUNCH("gemm_bf16");
  return TCAVT_OK;
}

}  // namespace tcavt
