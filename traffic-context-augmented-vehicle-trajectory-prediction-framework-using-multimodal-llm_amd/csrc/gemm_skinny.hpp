// The skinny GEMM form (M <= 32 rows: the decode step), auto-selected by tcavt_gemm_bf16 for tile code 0.
#pragma once
#include "gemm_epilogue.hpp"
#include <type_traits>

namespace tcavt {

// ===========================================================================
// Skinny form (M <= 32 rows: the decode step of text generation, one row per sample).  The contraction is a stream of
// the weight matrix through the chip, HBM-bound; the 256-row tiles above would leave all but a handful of CUs idle
// (N / 128 workgroups) and spend 8x the MFMA work on padding rows.  Here a workgroup owns NCB blocks of 16 output
// columns and ALL rows; its eight waves split K, each streaming its slice of the 16 x K weight panel straight from
// global memory into MFMA A fragments (16 bytes per lane, 64 contiguous bytes per weight row and instruction), with the
// <= 32 activation rows (L2-resident) as B fragments; the eight partial accumulators meet in LDS and are added in wave
// order (bit-reproducible).  Epilogues as above; TCAVT_EPI_NORM_OUT writes one partial sum of squares per workgroup
// (16 columns): norm_out_npart() in common.hpp tells producers and consumers the count.
// ===========================================================================
template <bool F16>
__device__ __forceinline__ f32x4 mfma16(const u32x4& a, const u32x4& b, const f32x4& c) {
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

constexpr int SK_WAVES = 8;

// FP8 weight stream (tcavt_gemm_args.w_layout = TCAVT_W_FRAG8, tcavt.h: tcavt_pack_weight8): a lane's eight e4m3 codes of a k-step
// (8 bytes) -> the 16-byte MFMA operand, four v_cvt_scalef32_pk_{f16,bf16}_fp8 at scale 1 (exact: every e4m3 value is an f16 and
// a bf16 value).  The power-of-two row scale is applied to the fp32 accumulators, not here.
template <bool F16>
__device__ __forceinline__ u32x4 fp8x8_to16(const u32x2& v) {
  u32x4 o;
  if constexpr (F16) {
    o[0] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(v[0], 1.0f, false));
    o[1] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(v[0], 1.0f, true));
    o[2] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(v[1], 1.0f, false));
    o[3] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(v[1], 1.0f, true));
  } else {
    o[0] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v[0], 1.0f, false));
    o[1] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v[0], 1.0f, true));
    o[2] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v[1], 1.0f, false));
    o[3] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v[1], 1.0f, true));
  }
  return o;
}

// agent-scope store / load of four floats (relaxed atomics: global_store / global_load ... sc1, coherent across the XCDs)
__device__ __forceinline__ void sk_store(float* ptr, f32x4 v) {
#pragma unroll
  for (int i = 0; i < 4; ++i) __hip_atomic_store(ptr + i, v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ f32x4 sk_load(const float* ptr) {
  f32x4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = __hip_atomic_load(ptr + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return v;
}

template <int EPI, int NCB, bool F16, bool NT, bool W8 = false>
__global__ __launch_bounds__(SK_WAVES * 64) void gemm_skinny_kernel(GemmP p) {
  __shared__ f32x4 red[SK_WAVES][NCB * 2][64];
  // fused LoRA down-projection, consumer side (RoPE form): group sums of the partials, then t as 16-bit rows [32][32]
  __shared__ float lp_sum[EPI == EPI_ROPE ? 512 : 1];
  __shared__ __attribute__((aligned(16))) bf16_t lp_t[EPI == EPI_ROPE ? 32 * 32 : 8];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool lp_in = EPI == EPI_ROPE && p.lp_np > 0;
  if constexpr (EPI == EPI_ROPE) {
    if (lp_in) reinterpret_cast<unsigned int*>(lp_t)[threadIdx.x] = 0u;  // 512 threads x 4 B = the whole tile
  }
  // Split K (p.sk_split = S > 1): the S slices of one column block get ids that are congruent mod 8 -- workgroups are dealt
  // round-robin to the 8 XCDs, so the slabs the last arriver reads were written through its own XCD's L2 (a speed choice
  // only: the hand-off below is correct for any placement).  Host: (number of column blocks) % 8 == 0 when S > 1.
  const int S = p.sk_split;
  int blk = blockIdx.x, ks = 0, mrow0 = 0;
  if (S > 1) {
    const int q = blockIdx.x >> 3;
    ks = q % S;
    blk = (q / S) * 8 + (blockIdx.x & 7);
  } else if (p.sk_msplit > 1) {  // (the two token blocks of a column block: ids congruent mod 8 -> one XCD, the weights' second read is an L2 hit)
    const int q = blockIdx.x >> 3;
    mrow0 = 16 * (q & 1);
    blk = (q >> 1) * 8 + (blockIdx.x & 7);
  }
  const int n0 = blk * (16 * NCB);
  const int r16 = lane & 15, kq = lane >> 4;
  // first output column of column block c.  RoPE: a workgroup owns the two 16-column blocks of one head that rotate
  // together (dimensions d and d + 32), so that two workgroups share a head (96 workgroups for the fused q|k|v instead of 48)
  int ncol[NCB];
#pragma unroll
  for (int c = 0; c < NCB; ++c)
    ncol[c] = EPI == EPI_ROPE ? (blk >> 1) * 64 + (blk & 1) * 16 + c * 32 : n0 + c * 16;
  f32x4 acc[NCB][2];
#pragma unroll
  for (int c = 0; c < NCB; ++c) acc[c][0] = acc[c][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  // this wave's K slice: K / (8 S) (a multiple of 32), 32 per MFMA step
  const int kper = p.K / (SK_WAVES * S);
  const int kbeg = (ks * SK_WAVES + wave) * kper;
  // Weight fragments: row-major W -> 16 rows x 64 bytes per instruction, K * 2 bytes apart; fragment-major copy (w_frag,
  // tcavt_pack_weight16) -> the same 1 KiB as consecutive bytes, the wave's K slice one contiguous run (k advances 16 x as fast)
  // FP8 copy (W8, tcavt_pack_weight8): the fragment-major order at one byte per element -- 512 bytes per k-step, 8 per lane;
  // the N fp32 row scales follow the N * K codes
  const bf16_t* wp[NCB];
  const int wstep = p.w_frag ? 16 : 1;
#pragma unroll
  for (int c = 0; c < NCB; ++c) {
    if constexpr (W8) wp[c] = reinterpret_cast<const bf16_t*>(reinterpret_cast<const char*>(p.W) + (long)ncol[c] * p.K + (long)kbeg * 16 + lane * 8);
    else wp[c] = p.w_frag ? p.W + (long)ncol[c] * p.K + (long)kbeg * 16 + lane * 8 : p.W + (long)(ncol[c] + r16) * p.ldw + kbeg + kq * 8;
  }
  f32x4 wsc[W8 ? NCB : 1];  // W8: the row scales 2^k of this lane's four output columns per column block
  const bf16_t* xp0 = p.A + (long)min(mrow0 + r16, p.M - 1) * p.lda + kbeg + kq * 8;
  const bf16_t* xp1 = p.A + (long)min(16 + r16, p.M - 1) * p.lda + kbeg + kq * 8;
  // fragment-major activations: the 16 tokens' fragments of a k-step are one 1 KiB run as well (rows >= M of a block hold
  // whatever the producer left: they only reach output columns >= M, which nobody stores)
  // (one block of 8 tokens, M <= 8: a k-step is 512 bytes, lanes r and r + 8 read the same 16)
  const int xstep = p.a_frag == 2 ? 8 : p.a_frag ? 16 : 1;
  if (p.a_frag == 2) {
    xp0 = p.A + (long)kbeg * 8 + kq * 64 + (r16 & 7) * 8;
  } else if (p.a_frag) {
    xp0 = p.A + (long)mrow0 * p.K + (long)kbeg * 16 + lane * 8;
    xp1 = p.A + (long)16 * p.K + (long)kbeg * 16 + lane * 8;
  }
  const bool two = p.M > 16 && p.sk_msplit <= 1;
  constexpr int U = 4;  // k-steps in flight (8 made the decode step slower: 3.08 vs 2.60 ms in round 2, and again in round 3 for the residual forms alone: 1.155 vs 1.138; so did 16 waves with K / 16 slices each: 1.55 vs 1.34 ms;
                        // FP8 weights, whose 8 k-steps hold the bytes of 4 here: 0.782 vs 0.757 ms at B = 8, 0.971 vs 0.941 at B = 32 --
                        // the converted operands cost the registers the narrower loads save, occupancy 3 instead of 4)
  // Epilogue operands of the two finishing waves (wave mb completes token block mb), fetched while the first batch of weight
  // loads is in flight instead of after the K loop: the row scale's partial sums, the RoPE position -> cos / sin rows, the
  // 16-bit residual, and (wave 0) the LoRA second source.  Each of these was one more dependent global-memory round trip
  // at the tail of a kernel that is a few microseconds long (decode step).
  const int pm = mrow0 + wave * 16 + r16;  // (meaningful for wave < 2)
  const long pmm = pm < p.M ? pm : 0;
  float rs = 1.f;
  f32x4 rope_c = {1.f, 1.f, 1.f, 1.f}, rope_s = {0.f, 0.f, 0.f, 0.f};
  u32x2 old16[NCB];
  u32x4 l_a0[2], l_a1[2], l_w[2][NCB];
  // Row scale of the fused RMSNorm (finishing waves): the H / 16 partial sums of a token are split over the four lanes that
  // share it (kq), eight quads each and ALL requested before the first weight batch -- row_rscale's index-order loop was four
  // dependent round trips at the head of a launch that lasts ten microseconds.  (Sum order: per lane in index order, then
  // the four lanes; the tiled kernels add in index order throughout -- same value up to fp32 summation order.)
  constexpr bool RSK = EPI == EPI_SILU || EPI == EPI_ROPE;
  f32x4 rsq[RSK ? 8 : 1];
  int rope_pos_v = 0;
  if constexpr (RSK) {
    if (wave < 2 && p.rs_part) {
      const f32x4* q = reinterpret_cast<const f32x4*>(p.rs_part + pmm * p.rs_npart);
      const int nq4 = p.rs_npart >> 2, per = (nq4 + 3) >> 2;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int idx = kq * per + i;
        rsq[i] = q[min(idx, nq4 - 1)];
        if (i >= per || idx >= nq4) rsq[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    if constexpr (EPI == EPI_ROPE) {
      if (wave < 2) rope_pos_v = p.rope_pos ? p.rope_pos[pmm] : (int)(pmm % p.rope_L);
    }
  }
  constexpr bool NORMF = EPI == EPI_NORM || EPI == EPI_NORM16;
  u32x2 lp_af[NORMF ? NCB : 1][NORMF ? 16 : 1];  // producer: this lane's 4 columns of the 16 adapter rows
  // fused LoRA down-projection, consumer side: t = lp_scale * sum of the lp_np partials the previous residual GEMM left --
  // value (m, j) by thread m * 16 + j of group g, groups of lp_np / G consecutive partials (G = a power of two that divides
  // lp_np), combined in group order (this workgroup's tokens: all M, or the 16-token block it owns when the token blocks
  // are split, sk_msplit).  The first 32 partials of a thread are requested HERE, before the first weight batch (they are
  // back before it; added up under it), the rest (M > 8) in the same place as before
  float lp_tv[EPI == EPI_ROPE ? 32 : 1];
  const float* lp_src = nullptr;
  int lp_per = 0, lp_nall = 0;
  if constexpr (EPI == EPI_ROPE) {
    if (lp_in) {
      const int mtok = p.sk_msplit > 1 ? min(16, p.M - mrow0) : p.M;
      const int nv = mtok * 16;
      lp_nall = p.M * 16;
      int G = 1;
      while (2 * G * nv <= SK_WAVES * 64 && p.lp_np % (2 * G) == 0) G *= 2;
      const int tid = threadIdx.x;
      if (tid < G * nv) {
        const int g = tid / nv, v = tid - g * nv;
        lp_per = p.lp_np / G;
        lp_src = p.lp_part + (long)g * lp_per * lp_nall + mrow0 * 16 + v;
#pragma unroll
        for (int u = 0; u < 32; ++u) lp_tv[u] = lp_src[(long)min(u, lp_per - 1) * lp_nall];
      }
    }
  }
  for (int k = 0; k < kper; k += 32 * U) {
    typedef typename std::conditional<W8, u32x2, u32x4>::type wfrag_t;
    wfrag_t wf[U][NCB];
    u32x4 x0[U], x1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + 32 * u < kper) {
#pragma unroll
        for (int c = 0; c < NCB; ++c) {
          const wfrag_t* wsrc;
          if constexpr (W8) wsrc = reinterpret_cast<const wfrag_t*>(reinterpret_cast<const char*>(wp[c]) + (k + 32 * u) * 16);
          else wsrc = reinterpret_cast<const wfrag_t*>(wp[c] + (k + 32 * u) * wstep);
          wf[u][c] = NT ? __builtin_nontemporal_load(wsrc) : *wsrc;
        }
        x0[u] = *reinterpret_cast<const u32x4*>(xp0 + (k + 32 * u) * xstep);
        if (two) x1[u] = *reinterpret_cast<const u32x4*>(xp1 + (k + 32 * u) * xstep);
      }
    }
    if constexpr (EPI == EPI_ROPE) {
      if (k == 0 && lp_src) {
        float acc_t = 0.f;
#pragma unroll
        for (int u = 0; u < 32; ++u) acc_t += u < lp_per ? lp_tv[u] : 0.f;
        for (int i = 32; i < lp_per; i += 32) {
          float tv[32];
#pragma unroll
          for (int u = 0; u < 32; ++u) tv[u] = lp_src[(long)min(i + u, lp_per - 1) * lp_nall];
#pragma unroll
          for (int u = 0; u < 32; ++u) acc_t += i + u < lp_per ? tv[u] : 0.f;
        }
        lp_sum[threadIdx.x] = acc_t;
      }
    }
    if constexpr (W8) {  // (every wave scales its own partial sums: requested under the first weight batch)
      if (k == 0) {
        const char* sc = reinterpret_cast<const char*>(p.W) + (long)p.N * p.K;
#pragma unroll
        for (int c = 0; c < NCB; ++c) wsc[c] = *reinterpret_cast<const f32x4*>(sc + (long)(ncol[c] + 4 * kq) * 4);
      }
    }
    if (k == 0 && wave < 2) {
      if constexpr (EPI == EPI_SILU || EPI == EPI_ROPE) {
        if (p.rs_part) {
          const int nq4 = p.rs_npart >> 2, per = (nq4 + 3) >> 2;
          float ss = 0.f;
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            ss += rsq[i][0];
            ss += rsq[i][1];
            ss += rsq[i][2];
            ss += rsq[i][3];
          }
          if (per > 8) {  // (more than 128 partials per row: the rest in further batches)
            const f32x4* q = reinterpret_cast<const f32x4*>(p.rs_part + pmm * p.rs_npart);
            for (int i = 8; i < per; ++i) {
              const int idx = kq * per + i;
              if (idx < nq4) {
                const f32x4 v4 = q[idx];
                ss += v4[0];
                ss += v4[1];
                ss += v4[2];
                ss += v4[3];
              }
            }
          }
          ss += __shfl_xor(ss, 16, 64);
          ss += __shfl_xor(ss, 32, 64);
          rs = rsqrtf(ss * p.rs_inv_h + p.rs_eps);
        }
      }
      if constexpr (EPI == EPI_ROPE) {
        if (ncol[0] < p.rope_cols) {
          const int pos = rope_pos_v;
          const int d = (blk & 1) * 16 + 4 * kq;
          rope_c = *reinterpret_cast<const f32x4*>(p.cosT + pos * 32 + d);
          rope_s = *reinterpret_cast<const f32x4*>(p.sinT + pos * 32 + d);
        }
        if (lp_in) {
          // (the partial sums: below, by all eight waves)
          if (wave == 0) {
#pragma unroll
            for (int c = 0; c < NCB; ++c) l_w[0][c] = *reinterpret_cast<const u32x4*>(p.W2 + (long)(ncol[c] + r16) * p.ldw2 + kq * 8);
          }
        } else if (wave == 0 && p.K2 > 0 && ks == 0) {  // (the second K source is added once: by slice 0)
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            if (32 * u < p.K2) {
              l_a0[u] = *reinterpret_cast<const u32x4*>(p.A2 + (long)min(mrow0 + r16, p.M - 1) * p.lda2 + 32 * u + kq * 8);
              l_a1[u] = *reinterpret_cast<const u32x4*>(p.A2 + (long)min(16 + r16, p.M - 1) * p.lda2 + 32 * u + kq * 8);
#pragma unroll
              for (int c = 0; c < NCB; ++c)
                l_w[u][c] = *reinterpret_cast<const u32x4*>(p.W2 + (long)(ncol[c] + r16) * p.ldw2 + 32 * u + kq * 8);
            }
          }
        }
      }
      if constexpr (EPI == EPI_NORM16) {
        if (p.flags & TCAVT_EPI_RESIDUAL) {
#pragma unroll
          for (int c = 0; c < NCB; ++c)
            old16[c] = *reinterpret_cast<const u32x2*>(p.res16 + (p.o_frag ? frag_off((int)pmm, n0 + c * 16 + 4 * kq, p.N, p.o_frag)
                                                                            : pmm * p.ldc + n0 + c * 16 + 4 * kq));
        }
      }
      if constexpr (NORMF) {
        if (p.lp_a) {
#pragma unroll
          for (int c = 0; c < NCB; ++c)
#pragma unroll
            for (int j = 0; j < 16; ++j)
              lp_af[c][j] = *reinterpret_cast<const u32x2*>(p.lp_a + (long)(j < 8 ? j : 8 + j) * p.lp_lda + n0 + c * 16 + 4 * kq);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + 32 * u < kper) {
#pragma unroll
        for (int c = 0; c < NCB; ++c) {
          u32x4 wv;
          if constexpr (W8) wv = fp8x8_to16<F16>(wf[u][c]);
          else wv = wf[u][c];
          acc[c][0] = mfma16<F16>(wv, x0[u], acc[c][0]);
          if (two) acc[c][1] = mfma16<F16>(wv, x1[u], acc[c][1]);
        }
      }
    }
  }
  // W8: the codes' partial sums times the rows' power-of-two scales (exact) -- here, before the 16-bit LoRA term below and the
  // reductions, so that every later step sees what the 16-bit path computes on the dequantised matrix, bit for bit
  if constexpr (W8) {
#pragma unroll
    for (int c = 0; c < NCB; ++c) {
      acc[c][0] *= wsc[c];
      acc[c][1] *= wsc[c];
    }
  }
  if constexpr (EPI == EPI_ROPE) {
    if (lp_in) {  // (uniform) fused LoRA down-projection: group sums -> t rows in LDS -> wave 0's B fragments, one 32-deep step
      __syncthreads();
      const int mtok = p.sk_msplit > 1 ? min(16, p.M - mrow0) : p.M;  // (t rows in LDS: local token index)
      const int nv = mtok * 16;
      if ((int)threadIdx.x < nv) {
        int G = 1;
        while (2 * G * nv <= SK_WAVES * 64 && p.lp_np % (2 * G) == 0) G *= 2;
        float tot = lp_sum[threadIdx.x];
        for (int g = 1; g < G; ++g) tot += lp_sum[g * nv + threadIdx.x];
        const int m_ = threadIdx.x >> 4, j = threadIdx.x & 15;
        lp_t[m_ * 32 + (j < 8 ? j : 8 + j)] = to16<F16>(tot * p.lp_scale);
      }
      __syncthreads();
      if (wave == 0 && ks == 0) {
        const u32x4 a0 = *reinterpret_cast<const u32x4*>(lp_t + min(r16, mtok - 1) * 32 + kq * 8);
        const u32x4 a1 = *reinterpret_cast<const u32x4*>(lp_t + min(16 + r16, mtok - 1) * 32 + kq * 8);
#pragma unroll
        for (int c = 0; c < NCB; ++c) {
          acc[c][0] = mfma16<F16>(l_w[0][c], a0, acc[c][0]);
          if (two) acc[c][1] = mfma16<F16>(l_w[0][c], a1, acc[c][1]);
        }
      }
    }
  }
  if constexpr (EPI == EPI_ROPE) {  // LoRA second K source (K2 = 64: two steps), done by wave 0 (of slice 0)
    if (!lp_in && p.K2 > 0 && wave == 0 && ks == 0) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {  // the first two steps come from the registers filled under the first weight batch
        if (32 * u < p.K2) {
#pragma unroll
          for (int c = 0; c < NCB; ++c) {
            acc[c][0] = mfma16<F16>(l_w[u][c], l_a0[u], acc[c][0]);
            if (two) acc[c][1] = mfma16<F16>(l_w[u][c], l_a1[u], acc[c][1]);
          }
        }
      }
      for (int k = 64; k < p.K2; k += 32) {
        const u32x4 a0 = *reinterpret_cast<const u32x4*>(p.A2 + (long)min(mrow0 + r16, p.M - 1) * p.lda2 + k + kq * 8);
        const u32x4 a1 = *reinterpret_cast<const u32x4*>(p.A2 + (long)min(16 + r16, p.M - 1) * p.lda2 + k + kq * 8);
#pragma unroll
        for (int c = 0; c < NCB; ++c) {
          const u32x4 w2 = *reinterpret_cast<const u32x4*>(p.W2 + (long)(ncol[c] + r16) * p.ldw2 + k + kq * 8);
          acc[c][0] = mfma16<F16>(w2, a0, acc[c][0]);
          if (two) acc[c][1] = mfma16<F16>(w2, a1, acc[c][1]);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NCB; ++c) {
    red[wave][c * 2][lane] = acc[c][0];
    red[wave][c * 2 + 1][lane] = acc[c][1];
  }
  __syncthreads();
  const bool finisher = wave == 0 || (wave == 1 && two);
  if (S <= 1 && !finisher) return;
  // ---- wave mb (0 / 1) finishes token block mb: lane holds features 4 (lane >> 4) .. + 3 of every column block for
  // token m = 16 mb + (lane & 15); the partials are added in wave order
  const int mb = wave & 1;
  const int m = mrow0 + mb * 16 + r16, nq = 4 * kq;
  const bool rowok = m < p.M;
  const long mm = rowok ? m : 0;
  f32x4 v[NCB];
  if (finisher) {
#pragma unroll
    for (int c = 0; c < NCB; ++c) {
      f32x4 t = red[0][c * 2 + mb][lane];
#pragma unroll
      for (int w = 1; w < SK_WAVES; ++w) t += red[w][c * 2 + mb][lane];
      v[c] = t;
    }
  }
  if (S > 1) {
    // ---- cross-workgroup combine: every slice writes its partial sums to its slab, every storing wave drains its stores,
    // barrier, ONE agent-scope ticket; the workgroup that draws S - 1 adds the S slabs in slice order (bit-reproducible
    // whatever the arrival order) and runs the epilogue.  The counter is re-armed by the last arriver (zeroed once by the
    // caller before first use).  The slabs move with agent-scope (sc1) stores and loads -- write-through to / read from the
    // point where the 8 XCDs' L2s agree -- and the order "slab stores complete -> ticket" is the s_waitcnt + barrier: the
    // release / acquire FENCES that plain stores would need write back and invalidate a whole L2 per workgroup
    // (buffer_wbl2 / buffer_inv: measured + 10 us per launch, twice what the split gains).
    float* slab = p.sk_slab + ((long)(blk * S + ks) * 2 * NCB) * 256;  // [mb][c][64 lanes][4]
    if (finisher) {
#pragma unroll
      for (int c = 0; c < NCB; ++c) sk_store(slab + ((mb * NCB + c) * 64 + lane) * 4, v[c]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int* last_flag = reinterpret_cast<int*>(&red[0][0][0]);  // (the one LDS array: all waves are past their reads of it)
    if (threadIdx.x == 0) {
      const int ticket = __hip_atomic_fetch_add(p.sk_cnt + blk, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = ticket == S - 1;
      if (last) __hip_atomic_store(p.sk_cnt + blk, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm for the next launch
      *last_flag = last;
    }
    __syncthreads();
    if (*last_flag == 0 || !finisher) return;
    const float* base = p.sk_slab + ((long)(blk * S) * 2 * NCB) * 256;
    f32x4 part[NCB];
#pragma unroll
    for (int c = 0; c < NCB; ++c) v[c] = sk_load(base + ((mb * NCB + c) * 64 + lane) * 4);
    for (int s2 = 1; s2 < S; ++s2) {
#pragma unroll
      for (int c = 0; c < NCB; ++c) part[c] = sk_load(base + (long)s2 * 2 * NCB * 256 + ((mb * NCB + c) * 64 + lane) * 4);
#pragma unroll
      for (int c = 0; c < NCB; ++c) v[c] += part[c];
    }
  }
  constexpr int OUT16 = F16 ? TCAVT_F16 : TCAVT_BF16;
  if constexpr (EPI == EPI_GENERIC) {
    if (!rowok) return;
#pragma unroll
    for (int c = 0; c < NCB; ++c) store_quad(p, m, n0 + c * 16 + nq, v[c] * p.acc_scale);
  } else if constexpr (EPI == EPI_NORM || EPI == EPI_NORM16) {
    const bool res = p.flags & TCAVT_EPI_RESIDUAL;
    float ss = 0.f;
    f32x4 hq[NCB];  // the 16-bit stream's values (what the next layer's projections read)
#pragma unroll
    for (int c = 0; c < NCB; ++c) {
      f32x4 o = v[c];
      const long off = mm * p.ldc + n0 + c * 16 + nq;
      if constexpr (EPI == EPI_NORM16) {  // 16-bit residual stream: in place, sums of the rounded values (see gemm_epilogue)
        f32x4 oldv = {0.f, 0.f, 0.f, 0.f};
        if (res) {
          const u32x2 old = old16[c];
          oldv = f32x4{from16_lo<F16>(old[0]), from16_hi<F16>(old[0]), from16_lo<F16>(old[1]), from16_hi<F16>(old[1])};
        }
        o = fma4(o, p.norm_scale, oldv);
        const u32x2 w = u32x2{pack16x2<F16>(o[0], o[1]), pack16x2<F16>(o[2], o[3])};
        if (rowok) *reinterpret_cast<u32x2*>(p.norm_h16 + (p.o_frag ? frag_off(m, n0 + c * 16 + nq, p.N, p.o_frag) : off)) = w;
        o = f32x4{from16_lo<F16>(w[0]), from16_hi<F16>(w[0]), from16_lo<F16>(w[1]), from16_hi<F16>(w[1])};
        hq[c] = o;
      } else {
        if (res) o += *reinterpret_cast<const f32x4*>(p.residual + mm * p.ldr + n0 + c * 16 + nq);
        if (rowok) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + off) = o;
        o *= p.norm_scale;  // (the 16-bit copy and the sums below are kept at norm_scale)
        const u32x2 w = u32x2{pack16x2<F16>(o[0], o[1]), pack16x2<F16>(o[2], o[3])};
        if (rowok) *reinterpret_cast<u32x2*>(p.norm_h16 + off) = w;
        hq[c] = f32x4{from16_lo<F16>(w[0]), from16_hi<F16>(w[0]), from16_lo<F16>(w[1]), from16_hi<F16>(w[1])};
      }
      ss += o[0] * o[0];
      ss += o[1] * o[1];
      ss += o[2] * o[2];
      ss += o[3] * o[3];
    }
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    if (lane < 16 && rowok) {
      p.norm_part[(long)m * (p.N / (16 * NCB)) + blk] = ss;
      flag_nonfinite(p, ss);
    }
    if (p.lp_a) {  // (uniform) this workgroup's share of the next layer's LoRA down-projection
      float pj[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        float a_ = 0.f;
#pragma unroll
        for (int c = 0; c < NCB; ++c) {
          const u32x2 w = lp_af[c][j];
          a_ += hq[c][0] * from16_lo<F16>(w[0]);
          a_ += hq[c][1] * from16_hi<F16>(w[0]);
          a_ += hq[c][2] * from16_lo<F16>(w[1]);
          a_ += hq[c][3] * from16_hi<F16>(w[1]);
        }
        a_ += __shfl_xor(a_, 16, 64);
        a_ += __shfl_xor(a_, 32, 64);
        pj[j] = a_;
      }
      if (lane < 16 && rowok) {
        float* dst = p.lp_part + ((long)blk * p.M + m) * 16;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
          *reinterpret_cast<f32x4*>(dst + 4 * q4) = f32x4{pj[4 * q4], pj[4 * q4 + 1], pj[4 * q4 + 2], pj[4 * q4 + 3]};
      }
    }
  } else if constexpr (EPI == EPI_SILU) {
    static_assert(EPI != EPI_SILU || NCB == 2, "gate block + up block");
    if (!rowok) return;
    const f32x4 g = v[0] * rs, u = v[NCB - 1] * rs;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = silu_mul(g[e], u[e]);
    if (p.o_frag)  // (16-bit output of the operand type: checked by the host)
      *reinterpret_cast<u32x2*>(static_cast<bf16_t*>(p.C) + frag_off(m, (n0 >> 1) + nq, p.N >> 1, p.o_frag)) =
          u32x2{pack16x2<F16>(o[0], o[1]), pack16x2<F16>(o[2], o[3])};
    else store_quad(p, m, (n0 >> 1) + nq, o);
  } else {  // EPI_ROPE: dimensions d = 16 half + nq .. + 3 and d + 32 of one head
    static_assert(EPI != EPI_ROPE || NCB == 2, "two partner blocks per workgroup");
    if (!rowok) return;
    const bool rot = ncol[0] < p.rope_cols;
    f32x4 lo = v[0] * rs, hi = v[NCB - 1] * rs;
    if (rot) {
      const f32x4 c = rope_c, sn = rope_s;
      const f32x4 l2 = lo * c - hi * sn, h2 = hi * c + lo * sn;
      lo = l2;
      hi = h2;
    }
    store_quad(p, m, ncol[0] + nq, lo);
    store_quad(p, m, ncol[NCB - 1] + nq, hi);
  }
  (void)OUT16;
}

template <int EPI, int NCB, bool F16>
static int launch_skinny(const GemmP& p, hipStream_t stream) {
  GemmP q = p;
  const int nblk = p.N / (16 * NCB);  // (RoPE: N / 64 heads x 2 halves = N / 32)
  // split K over S workgroups per column block when the caller lent a workspace: the decode step's projections are streams of
  // their weights, and N / 16 workgroups of 8 waves (128 for N = 2048: half the CUs, 4 KB per wave in flight) cannot keep the
  // memory system busy -- S is chosen so that ~two workgroups per CU stream, each wave's K slice staying a multiple of 32
  int S = 1;
  if (p.sk_slab && p.sk_cnt && nblk % 8 == 0 && !p.lp_a && p.lp_np == 0) {
    static const int max_wg = [] { const char* e = getenv("TCAVT_SK_MAXWG"); return e ? atoi(e) : 640; }();
    while (S < 8 && nblk * S * 2 <= max_wg && p.K % (SK_WAVES * S * 2 * 32) == 0) S *= 2;
    if ((long)nblk * S * 2 * NCB * 256 * 4 > p.sk_slab_bytes || nblk > p.sk_cnt_n) S = 1;
  }
  q.sk_split = S;
  static const bool no_msplit = getenv("TCAVT_SK_NO_MSPLIT") != nullptr;  // (A/B switch)
  // (only where the column blocks alone leave CUs idle -- o, down, q|k|v: 96-128 of 256; with more workgroups than CUs the
  //  second read of every weight row costs more than the activation rows it saves: gate|up 25.8 -> 33.2 us, lm_head likewise)
  const int msplit = (S == 1 && p.M > 16 && nblk % 8 == 0 && nblk <= 256 && !no_msplit) ? 2 : 1;
  q.sk_msplit = msplit;
  // Non-temporal weight loads where every weight byte is read ONCE per launch (one workgroup per column block) from the
  // fragment-major copy: 0.925 -> 0.885 ms per decode step at B = 8.  (On row-major weights nt was slower, 1.15 vs 1.09 ms --
  // the two 64-byte halves of a 128-byte line are fetched by different instructions there; with the token blocks on two
  // workgroups the second reader wants the L2 copy.)
  static const bool no_nt = getenv("TCAVT_SK_NO_NT") != nullptr;  // (A/B switch)
  const dim3 grid(nblk * S * msplit), block(SK_WAVES * 64);
  if (q.w_frag == 2) {  // FP8 copy (TCAVT_W_FRAG8)
    if (msplit == 1 && !no_nt) hipLaunchKernelGGL((gemm_skinny_kernel<EPI, NCB, F16, true, true>), grid, block, 0, stream, q);
    else hipLaunchKernelGGL((gemm_skinny_kernel<EPI, NCB, F16, false, true>), grid, block, 0, stream, q);
  } else if (q.w_frag && msplit == 1 && !no_nt) hipLaunchKernelGGL((gemm_skinny_kernel<EPI, NCB, F16, true>), grid, block, 0, stream, q);
  else hipLaunchKernelGGL((gemm_skinny_kernel<EPI, NCB, F16, false>), grid, block, 0, stream, q);
  TCAVT_CHECK_LAUNCH("gemm_bf16(skinny)");
  return TCAVT_OK;
}

}  // namespace tcavt
