// The fused epilogues of the tiled GEMM kernels (gemm_tile8.hpp, gemm_w4.hpp): generic (bias / ReLU / residual / dropout),
// SiLU*up (+ saved pre-activations), its backward, RoPE, and the residual + RMSNorm-input forms.
#pragma once
#include "gemm_params.hpp"

namespace tcavt {

__device__ __forceinline__ void store_quad(const GemmP& p, int m, int n, f32x4 v) {
  if (p.out_kind == TCAVT_BF16) {
    u32x2 o = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
    *reinterpret_cast<u32x2*>(reinterpret_cast<bf16_t*>(p.C) + (long)m * p.ldc + n) = o;
  } else if (p.out_kind == TCAVT_F16) {
    u32x2 o = {pack_f16x2(v[0], v[1]), pack_f16x2(v[2], v[3])};
    *reinterpret_cast<u32x2*>(reinterpret_cast<bf16_t*>(p.C) + (long)m * p.ldc + n) = o;
  } else {
    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + (long)m * p.ldc + n) = v;
  }
}

// ---------------------------------------------------------------------------
// Epilogue shared by both main-loop variants.  acc[i][j] holds, for n-tile i and m-tile j of this
// wave, features n..n+3 (n = n_base + 16 i + 4 (lane >> 4)) of token m = m_base + 16 j + (lane & 15).
// ---------------------------------------------------------------------------
__device__ __forceinline__ float silu_mul(float g, float u) {
  // g * sigmoid(g) * u with v_exp_f32 + v_rcp_f32 (1 ulp each): an IEEE division here cost ~10 VALU
  // instructions per output, 128 outputs per lane, with nothing to overlap them (one tile per CU at a time)
  return g * __builtin_amdgcn_rcpf(1.f + __expf(-g)) * u;
}

typedef __attribute__((ext_vector_type(2))) float f32x2;

// silu(g) * u for the lane's four consecutive features, written on natural register pairs so that the products are
// v_pk_mul_f32 (two outputs per issue slot; left to itself the vectoriser paired (0,2),(1,3) and paid for it in v_mov and
// re-interleaving instructions: ~50 instructions per quad, this is ~24).  Same arithmetic, same order as silu_mul.
template <bool F16>
__device__ __forceinline__ u32x2 silu_mul_quad(const f32x4& g, const f32x4& u) {
  const f32x2 g0 = {g[0], g[1]}, g1 = {g[2], g[3]}, u0 = {u[0], u[1]}, u1 = {u[2], u[3]};
  const f32x2 t0 = g0 * -1.44269504088896340736f, t1 = g1 * -1.44269504088896340736f;  // __expf(-g) = exp2(-g log2 e)
  const f32x2 d0 = f32x2{__builtin_amdgcn_exp2f(t0[0]), __builtin_amdgcn_exp2f(t0[1])} + 1.f;
  const f32x2 d1 = f32x2{__builtin_amdgcn_exp2f(t1[0]), __builtin_amdgcn_exp2f(t1[1])} + 1.f;
  const f32x2 r0 = {__builtin_amdgcn_rcpf(d0[0]), __builtin_amdgcn_rcpf(d0[1])};
  const f32x2 r1 = {__builtin_amdgcn_rcpf(d1[0]), __builtin_amdgcn_rcpf(d1[1])};
  const f32x2 o0 = g0 * r0 * u0, o1 = g1 * r1 * u1;
  return u32x2{pack16x2<F16>(o0[0], o0[1]), pack16x2<F16>(o1[0], o1[1])};
}

// ---- 16-byte epilogue accesses -------------------------------------------------------------------------------------------
// A lane holds four consecutive features (8 bytes as 16-bit values) of one token per 16x16 MFMA tile; the lane 16 further on
// holds the next four.  v_permlane16_swap (odd 16-lane rows of the first operand <-> even rows of the second) applied to the
// packed quads of two column-adjacent tiles a, b leaves EIGHT consecutive features in every lane -- even rows: tile a,
// features 4q .. 4q+7; odd rows: tile b, features 4(q-1) .. 4(q-1)+7 -- i.e. one global_store_dwordx4 instead of two
// dwordx2 (the store tail of these epilogues is issue-bound: half the instructions, same bytes, same addresses).  The swap is
// an involution, so a 16-byte LOAD from the same address followed by the same swap returns the two quads.
__device__ __forceinline__ void swap16(unsigned& a, unsigned& b) {
  const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
  a = r[0];
  b = r[1];
}
// element offset of this lane's 16 bytes relative to column 0 of tile a (tile b follows at column 16)
__device__ __forceinline__ int pair16_off(int lane) {
  const int q = lane >> 4;
  return (q & 1) ? 16 + 4 * (q - 1) : 4 * q;
}
__device__ __forceinline__ void store_pair16(bf16_t* row_pair, int off, const u32x2& a, const u32x2& b) {
  unsigned a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
  swap16(a0, b0);
  swap16(a1, b1);
  *reinterpret_cast<u32x4*>(row_pair + off) = u32x4{a0, a1, b0, b1};
}
__device__ __forceinline__ void unswap_pair16(const u32x4& v, u32x2& a, u32x2& b) {
  unsigned a0 = v[0], a1 = v[1], b0 = v[2], b1 = v[3];
  swap16(a0, b0);
  swap16(a1, b1);
  a = u32x2{a0, a1};
  b = u32x2{b0, b1};
}

// WHOLE_ONLY: the caller guarantees whole tiles (the 4-wave kernel); the bounds-checked paths are compiled out where
// a fast path covers the form.
// F16: the operands' 16-bit type; the fast paths below write 16-bit outputs of that same type (OUT16).
// rs_lds (ROWSCALE, optional): the row scales of this wave's rows already in LDS (rs_lds[16 j + (lane & 15)] for m-tile j;
// the 4-wave kernel computes them once per output tile while the first operands are in flight); otherwise they are
// summed here from the partials, all TM rows' loads in flight together.
// pin_acc re-pins the accumulator registers behind element (i, j) in front of a row's arithmetic.
// res_lds (NORM16 in the 4-wave kernel, optional): the output tile's 16-bit residual already in LDS (gemm_w4.hpp, residual
// prefetch) -- this lane's 16 bytes of row j, tile pair k are at res_lds + (k >> 1) * res_half + j * 8192 + (k & 1) * 512;
// otherwise the epilogue loads the residual from p.res16 itself.
template <int TN, int TM>
__device__ __forceinline__ void pin_acc(f32x4 (&acc)[TN][TM], int i, int j) {
  asm volatile("" : "+a"(acc[i][j]));
}
template <int V>
struct int_c {
  static constexpr int value = V;
};
template <int TM, int TN, int EPI, bool WHOLE_ONLY = false, bool F16 = false>
__device__ __forceinline__ void gemm_epilogue(const GemmP& p, f32x4 (&acc)[TN][TM], int m_base, int n_base, int lane,
                                              const float* rs_lds = nullptr, const char* res_lds = nullptr, int res_half = 0) {
  constexpr int OUT16 = F16 ? TCAVT_F16 : TCAVT_BF16;
  float rsv[TM];
  if constexpr (EPI == EPI_SILU || EPI == EPI_SILU_SAVE || EPI == EPI_ROPE) {
    if (rs_lds) {
#pragma unroll
      for (int j = 0; j < TM; ++j) rsv[j] = rs_lds[j * 16 + (lane & 15)];
    } else if (p.rs_part) {
      // same summation order as row_rscale (four partials per step, in index order): bit-identical to the LDS path
      float ss[TM];
      const f32x4* q[TM];
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        ss[j] = 0.f;
        q[j] = reinterpret_cast<const f32x4*>(p.rs_part + (long)min(m_base + j * 16 + (lane & 15), p.M - 1) * p.rs_npart);
      }
      for (int i = 0; i < (p.rs_npart >> 2); ++i) {
#pragma unroll
        for (int j = 0; j < TM; ++j) {
          const f32x4 v = q[j][i];
          ss[j] += v[0];
          ss[j] += v[1];
          ss[j] += v[2];
          ss[j] += v[3];
        }
      }
#pragma unroll
      for (int j = 0; j < TM; ++j) rsv[j] = rsqrtf(ss[j] * p.rs_inv_h + p.rs_eps);
    } else {
#pragma unroll
      for (int j = 0; j < TM; ++j) rsv[j] = 1.f;
    }
  }
  // ---- epilogue: lane holds features n..n+3 of token m in acc[i][j]
  const int nq = 4 * (lane >> 4);
  const int ml = lane & 15;
  // Fast paths for the forms the decoder launches (whole wave tile inside the matrix): row pointers hoisted,
  // no per-quad flag tests -- the general path below costs ~55 instructions per quad, these ~8.
  const bool whole = WHOLE_ONLY || (m_base + TM * 16 <= p.M && n_base + TN * 16 <= p.N);  // wave-uniform
  if constexpr ((EPI == EPI_NORM || EPI == EPI_NORM16) && TN % 4 == 0) {
    // o_proj / down_proj of the decoder with the NEXT RMSNorm's input side fused in: besides the fp32 residual stream
    // the epilogue leaves its 16-bit copy (the next projection's A operand; gamma is folded into that projection's
    // weights) and, per 64-column group, the row's partial sum of squares -- the consumer adds the N / 64 partials in
    // index order and applies rsqrt(mean + eps) as a row scale (TCAVT_EPI_ROWSCALE).  No float atomics anywhere.
    // The residual loads and the stores go to the same buffer (in place), so the compiler keeps them in program order:
    // written load-add-store per group, every group cost one full memory latency (16 groups per wave, ~25 us per tile
    // with every CU in its epilogue at once).  Hence the loads are issued up front, D rows (m-tiles) ahead of their use:
    // all of them in the 4-wave kernel, whose accumulators sit in AGPRs and whose operand registers are dead by now.
    const bool res = p.flags & TCAVT_EPI_RESIDUAL;
    const int npart = p.N >> 6;
    if constexpr (EPI == EPI_NORM16) {
      // 16-bit residual stream (eval / frozen-decoder passes): norm_h16 IS the stream -- read, added to and rewritten in
      // place by the lane that owns the element; the partial sums are of the rounded values, i.e. of what the consumer
      // multiplies.  4 bytes per element instead of 10.
      if constexpr (WHOLE_ONLY) {  // (the 4-wave kernel is dispatched for ldc % 8 == 0 only: launch_w4)
        // 16-byte form (pair16 helpers above): the residual pieces are requested DW rows ahead of their use (TN / 2 loads
        // of 16 bytes per row: half the instructions of the 8-byte form for the same lines), the stores are 16 bytes as well
        // Residual already in LDS (res_lds): conflict-free 16-byte LDS reads two rows ahead deliver the same u32x4 the global
        // load would; nothing but stores is left in the vector-memory queue.  Same arithmetic in the same order either way.
        const int off16 = pair16_off(lane);
        u32x4 oldw[TM][TN / 2];
        auto fetchw = [&](int j) {
          const bf16_t* hrow = p.res16 + (long)(m_base + j * 16 + ml) * p.ldc + n_base + off16;
#pragma unroll
          for (int k = 0; k < TN / 2; ++k)
            oldw[j][k] = res ? *reinterpret_cast<const u32x4*>(hrow + k * 32) : u32x4{0u, 0u, 0u, 0u};
        };
        auto fetchl = [&](int j) {
#pragma unroll
          for (int k = 0; k < TN / 2; ++k)
            oldw[j][k] = *reinterpret_cast<const u32x4*>(res_lds + (k >> 1) * res_half + j * 8192 + (k & 1) * 512);
        };
        auto rows = [&](auto fetch, auto depth) {
        constexpr int DW = decltype(depth)::value;
#pragma unroll
        for (int j = 0; j < DW; ++j) fetch(j);
#pragma unroll
        for (int j = 0; j < TM; ++j) {
          if (j + DW < TM) fetch(j + DW < TM ? j + DW : 0);
          const long m = m_base + j * 16 + ml;
          bf16_t* hrow = p.norm_h16 + m * p.ldc + n_base;
#pragma unroll
          for (int i = 0; i < TN; ++i) pin_acc(acc, i, j);  // (see the SiLU epilogue: no hoisted accumulator reads)
#pragma unroll
          for (int g = 0; g < TN / 4; ++g) {
            float ss = 0.f;
#pragma unroll
            for (int k = g * 2; k < g * 2 + 2; ++k) {
              u32x2 o[2], w[2];
              unswap_pair16(oldw[j][k], o[0], o[1]);
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                const f32x4 v = fma4(acc[2 * k + h][j], p.norm_scale,
                                     f32x4{from16_lo<F16>(o[h][0]), from16_hi<F16>(o[h][0]), from16_lo<F16>(o[h][1]), from16_hi<F16>(o[h][1])});
                w[h] = u32x2{pack16x2<F16>(v[0], v[1]), pack16x2<F16>(v[2], v[3])};
                const float r0 = from16_lo<F16>(w[h][0]), r1 = from16_hi<F16>(w[h][0]), r2 = from16_lo<F16>(w[h][1]),
                            r3 = from16_hi<F16>(w[h][1]);
                ss += r0 * r0;
                ss += r1 * r1;
                ss += r2 * r2;
                ss += r3 * r3;
              }
              store_pair16(hrow + k * 32, off16, w[0], w[1]);
            }
            ss += __shfl_xor(ss, 16, 64);
            ss += __shfl_xor(ss, 32, 64);
            if (lane < 16) {
              p.norm_part[m * npart + ((n_base >> 6) + g)] = ss;
              flag_nonfinite(p, ss);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        };
        if (res_lds) rows(fetchl, int_c<(TM > 2 ? 2 : TM)>{});
        else rows(fetchw, int_c<(TM > 5 ? 5 : TM)>{});
        return;
      }
      // 8-wave kernels: bounds-checked 8-byte accesses, the residual quads one row ahead of their use
      constexpr int D = 1;
      u32x2 old[TM][TN];
      auto fetch = [&](int j) {
        const long m = m_base + j * 16 + ml;
        const long mm = m < p.M ? m : 0;
        const bf16_t* hrow = p.res16 + mm * p.ldc + n_base + nq;
#pragma unroll
        for (int i = 0; i < TN; ++i) {
          const bool colok = n_base + (i >> 2) * 64 < p.N;
          old[j][i] = (res && colok) ? *reinterpret_cast<const u32x2*>(hrow + i * 16) : u32x2{0u, 0u};
        }
      };
#pragma unroll
      for (int j = 0; j < D; ++j) fetch(j);
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        if (j + D < TM) fetch(j + D < TM ? j + D : 0);
        const long m = m_base + j * 16 + ml;
        const bool rowok = m < p.M;
        const long mm = rowok ? m : 0;  // (rows beyond M read row 0 and store nothing: the shuffles below need every lane)
        bf16_t* hrow = p.norm_h16 + mm * p.ldc + n_base + nq;
#pragma unroll
        for (int g = 0; g < TN / 4; ++g) {
          const bool colok = n_base + g * 64 < p.N;  // (N % 64 == 0: a group is inside or outside)
          float ss = 0.f;
#pragma unroll
          for (int i = g * 4; i < g * 4 + 4; ++i) {
            const u32x2 o = old[j][i];
            const f32x4 v = fma4(acc[i][j], p.norm_scale,
                                 f32x4{from16_lo<F16>(o[0]), from16_hi<F16>(o[0]), from16_lo<F16>(o[1]), from16_hi<F16>(o[1])});
            const u32x2 w = u32x2{pack16x2<F16>(v[0], v[1]), pack16x2<F16>(v[2], v[3])};
            if (rowok && colok) *reinterpret_cast<u32x2*>(hrow + i * 16) = w;
            const float r0 = from16_lo<F16>(w[0]), r1 = from16_hi<F16>(w[0]), r2 = from16_lo<F16>(w[1]), r3 = from16_hi<F16>(w[1]);
            ss += r0 * r0;
            ss += r1 * r1;
            ss += r2 * r2;
            ss += r3 * r3;
          }
          ss += __shfl_xor(ss, 16, 64);
          ss += __shfl_xor(ss, 32, 64);
          if (lane < 16 && rowok && colok) {
            p.norm_part[m * npart + ((n_base >> 6) + g)] = ss;
            flag_nonfinite(p, ss);
          }
        }
      }
      return;
    } else {
      constexpr int D = WHOLE_ONLY ? 2 : 1;
      f32x4 rv[TM][TN];
      auto fetch = [&](int j) {
        const long m = m_base + j * 16 + ml;
        const long mm = (WHOLE_ONLY || m < p.M) ? m : 0;
        const float* rrow = p.residual + mm * p.ldr + n_base + nq;
#pragma unroll
        for (int i = 0; i < TN; ++i) {
          const bool colok = WHOLE_ONLY || n_base + (i >> 2) * 64 < p.N;
          rv[j][i] = (res && colok) ? *reinterpret_cast<const f32x4*>(rrow + i * 16) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
      };
#pragma unroll
      for (int j = 0; j < D && j < TM; ++j) fetch(j);
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        if (j + D < TM) fetch(j + D < TM ? j + D : 0);
        const long m = m_base + j * 16 + ml;
        const bool rowok = WHOLE_ONLY || m < p.M;
        const long mm = rowok ? m : 0;  // (rows beyond M read row 0 and store nothing: the shuffles below need every lane)
        float* crow = reinterpret_cast<float*>(p.C) + mm * p.ldc + n_base + nq;
        bf16_t* hrow = p.norm_h16 + mm * p.ldc + n_base + nq;
        unsigned ovf = 0u;
#pragma unroll
        for (int g = 0; g < TN / 4; ++g) {
          const bool colok = WHOLE_ONLY || n_base + g * 64 < p.N;  // (N % 64 == 0: a group is inside or outside)
          float ss = 0.f;
#pragma unroll
          for (int i = g * 4; i < g * 4 + 4; ++i) {
            const f32x4 vt = acc[i][j] + rv[j][i];
            const f32x4 v = vt * p.norm_scale;  // (the 16-bit copy and its sums of squares are kept at norm_scale; 1: unchanged)
            const u32x2 w = u32x2{pack16x2<F16>(v[0], v[1]), pack16x2<F16>(v[2], v[3])};
            if (rowok && colok) {
              *reinterpret_cast<f32x4*>(crow + i * 16) = vt;
              *reinterpret_cast<u32x2*>(hrow + i * 16) = w;
            }
            if constexpr (F16) ovf |= half_is_inf2(w[0]) | half_is_inf2(w[1]);  // the fp32 value may be fine, its fp16 copy not
            ss += v[0] * v[0];
            ss += v[1] * v[1];
            ss += v[2] * v[2];
            ss += v[3] * v[3];
          }
          ss += __shfl_xor(ss, 16, 64);
          ss += __shfl_xor(ss, 32, 64);
          if (lane < 16 && rowok && colok) {
            p.norm_part[m * npart + ((n_base >> 6) + g)] = ss;
            flag_nonfinite(p, ss);
          }
        }
        if (F16 && ovf && rowok && p.nf_flag) atomicCAS(p.nf_flag, 0, p.nf_tag);
      }
      return;
    }
  }
  if constexpr (EPI == EPI_GENERIC) {
    if (whole && p.acc_scale == 1.f && p.out_kind == TCAVT_F32 && p.flags == TCAVT_EPI_RESIDUAL) {
      // (C and residual may be one buffer: load-add-store per quad would serialise on the memory latency -- a row's
      // residual quads are loaded together, one row ahead of their use)
      f32x4 rv[TM][TN];
      auto fetch = [&](int j) {
        const float* rrow = p.residual + (long)(m_base + j * 16 + ml) * p.ldr + n_base + nq;
#pragma unroll
        for (int i = 0; i < TN; ++i) rv[j][i] = *reinterpret_cast<const f32x4*>(rrow + i * 16);
      };
      fetch(0);
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        if (j + 1 < TM) fetch(j + 1 < TM ? j + 1 : 0);
        const long m = m_base + j * 16 + ml;
        float* crow = reinterpret_cast<float*>(p.C) + m * p.ldc + n_base + nq;
#pragma unroll
        for (int i = 0; i < TN; ++i) *reinterpret_cast<f32x4*>(crow + i * 16) = acc[i][j] + rv[j][i];
      }
      return;
    }
    if (whole && p.acc_scale == 1.f && p.out_kind == OUT16 && p.flags == 0) {
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        const long m = m_base + j * 16 + ml;
        bf16_t* crow = reinterpret_cast<bf16_t*>(p.C) + m * p.ldc + n_base + nq;
#pragma unroll
        for (int i = 0; i < TN; ++i) {
          const f32x4 v = acc[i][j];
          *reinterpret_cast<u32x2*>(crow + i * 16) = u32x2{pack16x2<F16>(v[0], v[1]), pack16x2<F16>(v[2], v[3])};
        }
      }
      return;
    }
  }
  if constexpr (EPI == EPI_SILUBWD) {
    // d(silu(gate) * up) straight from the accumulator of down_proj's dgrad GEMM (include/tcavt.h: TCAVT_EPI_SILU_BWD): for
    // the lane's four features of a 16-column tile, gate and up sit in two column-adjacent 16-column blocks of the
    // interleaved pre-activation row, and so do dgate and dup in the output row -- one 16-byte load and one 16-byte store
    // per tile (pair16 helpers above).  Same arithmetic as silu_mul_bwd_kernel, on the un-rounded d.
    static_assert(WHOLE_ONLY, "the SiLU-backward epilogue exists in the 4-wave kernel only");
    constexpr int DW = 2;  // rows of pre-activations requested ahead (TN x 16 bytes per lane and row)
    const int off16 = pair16_off(lane);
    u32x4 pre[TM][TN];
    auto fetchp = [&](int j) {
      const bf16_t* arow = p.aux + (long)(m_base + j * 16 + ml) * p.ldaux + 2 * n_base + off16;
#pragma unroll
      for (int i = 0; i < TN; ++i) pre[j][i] = *reinterpret_cast<const u32x4*>(arow + i * 32);
    };
#pragma unroll
    for (int j = 0; j < DW && j < TM; ++j) fetchp(j);
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      if (j + DW < TM) fetchp(j + DW < TM ? j + DW : 0);
      bf16_t* crow = reinterpret_cast<bf16_t*>(p.C) + (long)(m_base + j * 16 + ml) * p.ldc + 2 * n_base;
#pragma unroll
      for (int i = 0; i < TN; ++i) pin_acc(acc, i, j);  // (no hoisted accumulator reads: see the SiLU epilogue)
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        u32x2 gq, uq;
        unswap_pair16(pre[j][i], gq, uq);
        const f32x4 d = acc[i][j];
        float dg[4], du[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float g = (e & 1) ? from16_hi<F16>(gq[e >> 1]) : from16_lo<F16>(gq[e >> 1]);
          const float u = (e & 1) ? from16_hi<F16>(uq[e >> 1]) : from16_lo<F16>(uq[e >> 1]);
          const float sg = __builtin_amdgcn_rcpf(1.f + __expf(-g));
          dg[e] = d[e] * u * sg * (1.f + g * (1.f - sg));
          du[e] = d[e] * g * sg;
        }
        store_pair16(crow + i * 32, off16, u32x2{pack16x2<F16>(dg[0], dg[1]), pack16x2<F16>(dg[2], dg[3])},
                     u32x2{pack16x2<F16>(du[0], du[1]), pack16x2<F16>(du[2], du[3])});
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    return;
  }
  if constexpr ((EPI == EPI_SILU || EPI == EPI_SILU_SAVE) && TN % 4 == 0) {
    // (the 4-wave kernel is dispatched for this form only -- silu16_ok() on the host -- so that its general path, and
    // the registers it costs around the persistent loop, compile away)
    if (WHOLE_ONLY || (whole && p.out_kind == OUT16 && (p.ldc & 7) == 0)) {
      // two gate|up tile pairs -> two adjacent 16-column output tiles -> one 16-byte store per lane
      const int off16 = pair16_off(lane);
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        const long m = m_base + j * 16 + ml;
        bf16_t* crow = reinterpret_cast<bf16_t*>(p.C) + m * p.ldc + (n_base >> 1);
        const float rs = rsv[j];  // fused RMSNorm: 1 / rms of the row (gamma is in W)
        if constexpr (WHOLE_ONLY) {
          // (4-wave kernel: the accumulators live in AGPRs; re-pinning this row's here keeps their v_accvgpr_reads from
          // being hoisted over the rows before it -- 150 hoisted reads cost spills that were reloaded behind the stores)
#pragma unroll
          for (int i = 0; i < TN; ++i) pin_acc(acc, i, j);
        }
#pragma unroll
        for (int i = 0; i < TN; i += 4) {
          u32x2 o[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const f32x4 g = acc[i + 2 * h][j] * rs, u = acc[i + 2 * h + 1][j] * rs;
            if constexpr (EPI == EPI_SILU_SAVE) {
              bf16_t* arow = p.aux + m * p.ldaux + n_base + (i + 2 * h) * 16 + nq;
              *reinterpret_cast<u32x2*>(arow) = u32x2{pack16x2<F16>(g[0], g[1]), pack16x2<F16>(g[2], g[3])};
              *reinterpret_cast<u32x2*>(arow + 16) = u32x2{pack16x2<F16>(u[0], u[1]), pack16x2<F16>(u[2], u[3])};
            }
            o[h] = silu_mul_quad<F16>(g, u);
          }
          store_pair16(crow + (i >> 1) * 16, off16, o[0], o[1]);
        }
        // (one row of MFMA tiles at a time: left free, the scheduler hoists the accumulator reads of later rows over this
        // one's arithmetic, runs out of registers and spills -- and a scratch reload waits for every store issued so far)
        __builtin_amdgcn_sched_barrier(0);
      }
      return;
    }
  }
  if constexpr (EPI == EPI_SILU || EPI == EPI_SILU_SAVE) {
    if (whole && p.out_kind == OUT16) {
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        const long m = m_base + j * 16 + ml;
        bf16_t* crow = reinterpret_cast<bf16_t*>(p.C) + m * p.ldc + (n_base >> 1) + nq;
        const float rs = rsv[j];  // fused RMSNorm: 1 / rms of the row (gamma is in W)
#pragma unroll
        for (int i = 0; i < TN; i += 2) {
          const f32x4 g = acc[i][j] * rs, u = acc[i + 1][j] * rs;
          if constexpr (EPI == EPI_SILU_SAVE) {
            bf16_t* arow = p.aux + m * p.ldaux + n_base + i * 16 + nq;
            *reinterpret_cast<u32x2*>(arow) = u32x2{pack16x2<F16>(g[0], g[1]), pack16x2<F16>(g[2], g[3])};
            *reinterpret_cast<u32x2*>(arow + 16) = u32x2{pack16x2<F16>(u[0], u[1]), pack16x2<F16>(u[2], u[3])};
          }
          *reinterpret_cast<u32x2*>(crow + (i >> 1) * 16) =
              u32x2{pack16x2<F16>(silu_mul(g[0], u[0]), silu_mul(g[1], u[1])),
                    pack16x2<F16>(silu_mul(g[2], u[2]), silu_mul(g[3], u[3]))};
        }
      }
      return;
    }
  }
  if constexpr (EPI == EPI_ROPE && WHOLE_ONLY) {
    // 4-wave kernel (dispatched for 16-bit outputs of the operand type with ldc % 8 == 0 only): 16-byte stores (pair16 helpers above); the cos / sin
    // rows of one row of MFMA tiles are loaded one row ahead
    const int off16 = pair16_off(lane);
    f32x4 cs[2][2], sn[2][2];
    auto fetch = [&](int j, int slot) {
      const int m = m_base + j * 16 + ml;
      const int pos = p.rope_pos ? p.rope_pos[m] : m % p.rope_L;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        cs[slot][i] = *reinterpret_cast<const f32x4*>(p.cosT + pos * 32 + nq + i * 16);
        sn[slot][i] = *reinterpret_cast<const f32x4*>(p.sinT + pos * 32 + nq + i * 16);
      }
    };
    fetch(0, 0);
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      if (j + 1 < TM) fetch(j + 1 < TM ? j + 1 : 0, (j + 1) & 1);
      const int m = m_base + j * 16 + ml;
      bf16_t* crow = reinterpret_cast<bf16_t*>(p.C) + (long)m * p.ldc + n_base;
      const float rs = rsv[j];  // fused RMSNorm: 1 / rms of the row (gamma is in W)
#pragma unroll
      for (int i = 0; i < TN; ++i) pin_acc(acc, i, j);  // (see the SiLU epilogue: no hoisted accumulator reads)
#pragma unroll
      for (int hh = 0; hh < TN / 4; ++hh) {
        const bool rot = n_base + hh * 64 < p.rope_cols;  // uniform: q and k heads rotate, v heads do not
        u32x2 o[4];
        if (rot) {
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const f32x4 lo = acc[hh * 4 + i][j] * rs, hi = acc[hh * 4 + i + 2][j] * rs;
            const f32x4 c = cs[j & 1][i];
            const f32x4 s = sn[j & 1][i];
            const f32x4 l2 = lo * c - hi * s;
            const f32x4 h2 = hi * c + lo * s;
            o[i] = u32x2{pack16x2<F16>(l2[0], l2[1]), pack16x2<F16>(l2[2], l2[3])};
            o[i + 2] = u32x2{pack16x2<F16>(h2[0], h2[1]), pack16x2<F16>(h2[2], h2[3])};
          }
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const f32x4 v = acc[hh * 4 + i][j] * rs;
            o[i] = u32x2{pack16x2<F16>(v[0], v[1]), pack16x2<F16>(v[2], v[3])};
          }
        }
        store_pair16(crow + hh * 64, off16, o[0], o[1]);
        store_pair16(crow + hh * 64 + 32, off16, o[2], o[3]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    return;
  }
  if constexpr (EPI == EPI_ROPE) {
    if (whole && p.out_kind == OUT16) {
      // 8-wave kernels: cos / sin rows are loaded one row ahead of their use: issued between the stores of the output,
      // which the compiler must assume they alias, every load cost a full L2 latency (32 of them per tile)
      constexpr int D = 1;
      f32x4 cs[TM][2], sn[TM][2];
      int pos[TM];
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        const int m = m_base + j * 16 + ml;
        pos[j] = p.rope_pos ? p.rope_pos[m] : m % p.rope_L;
      }
      auto fetch = [&](int j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          cs[j][i] = *reinterpret_cast<const f32x4*>(p.cosT + pos[j] * 32 + nq + i * 16);
          sn[j][i] = *reinterpret_cast<const f32x4*>(p.sinT + pos[j] * 32 + nq + i * 16);
        }
      };
#pragma unroll
      for (int j = 0; j < D; ++j) fetch(j);
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        if (j + D < TM) fetch(j + D < TM ? j + D : 0);
        const int m = m_base + j * 16 + ml;
        bf16_t* crow = reinterpret_cast<bf16_t*>(p.C) + (long)m * p.ldc + n_base + nq;
        const float rs = rsv[j];  // fused RMSNorm: 1 / rms of the row (gamma is in W)
#pragma unroll
        for (int hh = 0; hh < TN / 4; ++hh) {
          const bool rot = n_base + hh * 64 < p.rope_cols;  // uniform: q and k heads rotate, v heads do not
          // (two separate bodies: merging rotated temporaries with the un-rotated accumulators in one variable made the
          // compiler shuttle ~1000 values through v_accvgpr_write / _mov per tile)
          if (rot) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
              const f32x4 lo = acc[hh * 4 + i][j] * rs, hi = acc[hh * 4 + i + 2][j] * rs;
              const f32x4 c = cs[j][i];
              const f32x4 s = sn[j][i];
              const f32x4 l2 = lo * c - hi * s;
              const f32x4 h2 = hi * c + lo * s;
              *reinterpret_cast<u32x2*>(crow + hh * 64 + i * 16) = u32x2{pack16x2<F16>(l2[0], l2[1]), pack16x2<F16>(l2[2], l2[3])};
              *reinterpret_cast<u32x2*>(crow + hh * 64 + 32 + i * 16) = u32x2{pack16x2<F16>(h2[0], h2[1]), pack16x2<F16>(h2[2], h2[3])};
            }
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const f32x4 v = acc[hh * 4 + i][j] * rs;
              *reinterpret_cast<u32x2*>(crow + hh * 64 + i * 16) = u32x2{pack16x2<F16>(v[0], v[1]), pack16x2<F16>(v[2], v[3])};
            }
          }
        }
      }
      return;
    }
  }
  if constexpr (EPI == EPI_NORM || EPI == EPI_NORM16) {
    return;  // (TN % 4 != 0: the 64x64 form, never dispatched for this epilogue)
  }
  if constexpr (EPI == EPI_GENERIC || EPI == EPI_DROP) {
    // Loads first, stores after: bias / residual loads written between the stores of C (which they may alias as far as
    // the compiler knows) each waited for a full memory latency, TM x TN times per wave.  The column biases are loaded
    // once, the row biases for all rows, the residual quads one row ahead of their use.
    const bool has_bias = p.flags & TCAVT_EPI_BIAS, has_brow = p.flags & TCAVT_EPI_BIAS_ROW, has_res = p.flags & TCAVT_EPI_RESIDUAL;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 bq[TN];
    float bm[TM];
#pragma unroll
    for (int i = 0; i < TN; ++i) {
      const int n = n_base + i * 16 + nq;
      bq[i] = (has_bias && n < p.N) ? *reinterpret_cast<const f32x4*>(p.bias + n) : zero4;
    }
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      const int m = m_base + j * 16 + ml;
      bm[j] = (has_brow && m < p.M) ? p.bias[m] : 0.f;
    }
    f32x4 rv[TM][TN];
    auto fetch = [&](int j) {
      const int m = m_base + j * 16 + ml;
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        const int n = n_base + i * 16 + nq;
        rv[j][i] = (has_res && m < p.M && n < p.N) ? *reinterpret_cast<const f32x4*>(p.residual + (long)m * p.ldr + n) : zero4;
      }
    };
    fetch(0);
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      if (j + 1 < TM) fetch(j + 1 < TM ? j + 1 : 0);
      const int m = m_base + j * 16 + ml;
      if (m >= p.M) continue;
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        const int n = n_base + i * 16 + nq;
        if (n >= p.N) continue;
        f32x4 v = acc[i][j] * p.acc_scale;
        if (has_bias) v += bq[i];
        if (has_brow) {
          v[0] += bm[j]; v[1] += bm[j]; v[2] += bm[j]; v[3] += bm[j];
        }
        if (p.flags & TCAVT_EPI_RELU) {
          v[0] = relu_nan(v[0]); v[1] = relu_nan(v[1]);
          v[2] = relu_nan(v[2]); v[3] = relu_nan(v[3]);
        }
        if constexpr (EPI == EPI_DROP) {
          float sc[4];
          dropout_quad(p.drop, ((unsigned long long)m * (unsigned long long)p.N + (unsigned long long)n) >> 2, sc);
          v[0] *= sc[0]; v[1] *= sc[1]; v[2] *= sc[2]; v[3] *= sc[3];
        }
        if (has_res) v += rv[j][i];
        store_quad(p, m, n, v);
      }
    }
  } else if constexpr (EPI == EPI_SILU || EPI == EPI_SILU_SAVE) {
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      const int m = m_base + j * 16 + ml;
      if (m >= p.M) continue;
#pragma unroll
      for (int i = 0; i < TN; i += 2) {
        if (n_base + i * 16 >= p.N) continue;  // partial last tile column
        const int n = ((n_base) >> 1) + (i >> 1) * 16 + nq;
        const float rs = rsv[j];
        const f32x4 g = acc[i][j] * rs, u = acc[i + 1][j] * rs;
        if constexpr (EPI == EPI_SILU_SAVE) {
          bf16_t* arow = p.aux + (long)m * p.ldaux + n_base + i * 16 + nq;
          *reinterpret_cast<u32x2*>(arow) = u32x2{pack16x2<F16>(g[0], g[1]), pack16x2<F16>(g[2], g[3])};
          *reinterpret_cast<u32x2*>(arow + 16) = u32x2{pack16x2<F16>(u[0], u[1]), pack16x2<F16>(u[2], u[3])};
        }
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = silu_mul(g[e], u[e]);
        store_quad(p, m, n, v);
      }
    }
  } else {  // EPI_ROPE
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      const int m = m_base + j * 16 + ml;
      if (m >= p.M) continue;
      const int pos = p.rope_pos ? p.rope_pos[m] : m % p.rope_L;
#pragma unroll
      for (int hh = 0; hh < TN / 4; ++hh) {
        const int nb = n_base + hh * 64;
        if (nb >= p.N) continue;  // partial last tile column (N % BN != 0)
        const bool rot = nb < p.rope_cols;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int d = i * 16 + nq;
          const float rs = rsv[j];
          f32x4 lo = acc[hh * 4 + i][j] * rs, hi = acc[hh * 4 + i + 2][j] * rs;
          if (rot) {
            const f32x4 c = *reinterpret_cast<const f32x4*>(p.cosT + pos * 32 + d);
            const f32x4 s = *reinterpret_cast<const f32x4*>(p.sinT + pos * 32 + d);
            const f32x4 l2 = lo * c - hi * s;
            const f32x4 h2 = hi * c + lo * s;
            lo = l2; hi = h2;
          }
          store_quad(p, m, nb + d, lo);
          store_quad(p, m, nb + 32 + d, hi);
        }
      }
    }
  }
}

}  // namespace tcavt
