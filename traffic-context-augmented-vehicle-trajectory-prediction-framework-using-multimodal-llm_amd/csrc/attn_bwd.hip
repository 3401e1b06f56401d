// Attention backward of the decoder layers (the walk that calls it: llm_backward.hip), on the matrix cores, nothing of
// S / P / dS stored.  Three pairs of a query-major kernel (row statistics, dQ) and a key-major one (dK, dV):
//   tiled     attn_bwd_scores_kernel + attn_bwd_dkv_kernel               any T, fp32 output (finished by rope_bwd_pack_kernel)
//   resident  attn_bwd_dq_kernel + attn_bwd_dkv_res_kernel               T <= 256, fp32 or rotated 16-bit output
//   chunked   attn_bwd_dq_long_kernel + attn_bwd_dkv_long_kernel         T <= 2048 in chunks of 256, rotated 16-bit output
// The GEMM-composed forms (llm_backward.attn_bwd_composed) and the scalar-FMA kernel are cross-checks: attn_bwd_check.hip.
#include <string>

#include "common.hpp"
#include <stdlib.h>

namespace tcavt {

// fp32 [M, ncols] gradient of the rotated q | k | v  ->  bf16 gradient of the projections' outputs: the first
// rope_cols columns (q and k heads, head_dim 64 each) get the transposed rotation
//   g_t1 = g_o1 * cos + g_o2 * sin,   g_t2 = g_o2 * cos - g_o1 * sin      (forward: o1 = t1 cos - t2 sin, o2 = t2 cos + t1 sin)
template <bool F16>
__global__ __launch_bounds__(256) void rope_bwd_pack_kernel(const float* __restrict__ g32, bf16_t* __restrict__ out,
                                                            const float* __restrict__ cosT, const float* __restrict__ sinT,
                                                            long M, int ncols, int rope_cols, int L) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;  // one thread per (row, column pair c / c + 32 of a head)
  const int half = ncols / 2;
  if (idx >= M * half) return;
  const long row = idx / half;
  const int p = (int)(idx - row * half);
  const int head = p >> 5, w = p & 31;
  const int c1 = head * 64 + w, c2 = c1 + 32;
  const float a = g32[row * ncols + c1], b = g32[row * ncols + c2];
  float o1 = a, o2 = b;
  if (c1 < rope_cols) {
    const int pos = (int)(row % L);
    const float cs = cosT[pos * 32 + w], sn = sinT[pos * 32 + w];
    o1 = a * cs + b * sn;
    o2 = b * cs - a * sn;
  }
  out[row * ncols + c1] = to16<F16>(o1);
  out[row * ncols + c2] = to16<F16>(o2);
}

// ---------------------------------------------------------------------------
// Scores on the matrix cores, fused with the softmax backward (the production form of the middle of the attention
// backward): one workgroup per (sample, query head, block of 64 queries); wave w owns 16 query rows and computes its
// 16 x 64 tiles of  S = q K^T  and  dP = dO V^T  with v_mfma_f32_16x16x32_bf16 (q, dO rows are the A fragments, held in
// registers; K / V blocks are staged through LDS one block ahead and give the B fragments), in two sweeps over the key blocks at
// or below the diagonal: row maxima, row sums and sum(P dP) (online softmax); then P and dS, which leave through LDS tiles as dS row-major
// and P^T, dS^T (as causal_softmax_bwd_tiles_kernel).  S and dP never exist in memory.
// D[m][n] of the MFMA sits in lane l as m = 4 (l >> 4) + e, n = l & 15.
// ---------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(256, 3) void attn_bwd_scores_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dO,
                                                              bf16_t* __restrict__ dS, bf16_t* __restrict__ PT,
                                                              bf16_t* __restrict__ dST, float* __restrict__ dQ, long ld_dq,
                                                              float* __restrict__ stats, const int* __restrict__ kv_len, int T,
                                                              int Tp, int nq, int nkv, float scale,
                                                              const float* __restrict__ lse, const bf16_t* __restrict__ att) {
  // lse + att (optional, both or neither): the forward's log-sum-exp per query row [B*nq*T] (tcavt_attn_causal_gqa_lse) and
  // its output [B*T, nq*64].  With them the row statistics are known before any key is read -- P = exp(s - lse), and
  // sum(P dP) = dO . O (the row of the output times the row of its gradient, as in FlashAttention-2's backward) -- so the
  // first of the two sweeps over the key blocks (S and dP on the matrix cores, for the maximum, the sum and sum(P dP)) is
  // not run: 3 instead of 5 block products per key block.
  // stats (optional, fp32 [B*nq*T, 4]): row maximum of the scaled scores, 1 / row sum, sum(P dP) -- what
  // attn_bwd_dkv_kernel needs to rebuild P and dS for its key block.  PT / dST (optional): only for the GEMM form of dK, dV.
  // dQ (optional, fp32 [B*T, ld_dq], head h at columns 64 h): dQ = dS K accumulated over the key blocks inside the last
  // sweep (A = the dS tile in LDS, B = a transposed copy of the K block); dS (optional): the row-major copy for an
  // external dQ product.
  __shared__ bf16_t tP[64][66], tD[64][66];
  __shared__ __attribute__((aligned(16))) bf16_t ksT[64][72];  // K block transposed [d][key] (last sweep, dQ only)
  const int nqb = Tp >> 6;
  const int qb = blockIdx.x % nqb;
  const long bh = blockIdx.x / nqb;
  const int b = (int)(bh / nq), h = (int)(bh % nq);
  const int j = h / (nq / nkv);
  const int klen = min(kv_len[b], T);
  const int q0 = qb * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const long nqkv = (long)(nq + 2 * nkv) * 64;
  const long row0 = (long)b * T;
  bf16x8 qf[2], gf[2];
  {
    const long ar = row0 + min(q0 + wave * 16 + l15, T - 1);  // rows >= T: clamped load, masked below (nv = 0)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      qf[kk] = *reinterpret_cast<const bf16x8*>(qkv + ar * nqkv + h * 64 + kk * 32 + l4 * 8);
      gf[kk] = *reinterpret_cast<const bf16x8*>(dO + ar * (long)(nq * 64) + h * 64 + kk * 32 + l4 * 8);
    }
  }
  int nv[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = q0 + wave * 16 + l4 * 4 + e;
    nv[e] = i < T ? min(i + 1, klen) : 0;
  }
  // K / V key blocks go global -> registers -> LDS with whole 128-byte rows per 8 lanes (coalesced), one block ahead of the
  // compute; the B fragments are then 16-byte LDS reads (rows padded to 144 bytes).  Loading the fragments straight from
  // global memory put every lane on its own cache line: 64 address cycles per load, 372 us per launch.
  __shared__ __attribute__((aligned(16))) bf16_t ks[64][72], vs[64][72];
  const int srow = threadIdx.x >> 2, sch = (threadIdx.x & 3) * 16;
  // transposed staging: the four threads of a source row write rows 16 apart, i.e. the same bank; the 16-byte column
  // chunk is therefore XOR-ed with the row's 16-block (= threadIdx.x & 3 for the writer, dt for the reader)
  const int tcol = (((srow >> 3) ^ (threadIdx.x & 3)) << 3) | (srow & 7);
  const bf16_t* kbase = qkv + (nq + j) * 64 + sch;
  const bf16_t* vbase = qkv + (nq + nkv + j) * 64 + sch;
  u32x4 kreg[2], vreg[2];
  auto fetch = [&](int kb, bool want_v) {
    const long kr = row0 + min(kb * 64 + srow, T - 1);  // keys >= T: clamped load, masked (>= nv)
    kreg[0] = *reinterpret_cast<const u32x4*>(kbase + kr * nqkv);
    kreg[1] = *reinterpret_cast<const u32x4*>(kbase + kr * nqkv + 8);
    if (want_v) {
      vreg[0] = *reinterpret_cast<const u32x4*>(vbase + kr * nqkv);
      vreg[1] = *reinterpret_cast<const u32x4*>(vbase + kr * nqkv + 8);
    }
  };
  bool want_t = false;
  auto stage = [&](bool want_v) {
    *reinterpret_cast<u32x4*>(&ks[srow][sch]) = kreg[0];
    *reinterpret_cast<u32x4*>(&ks[srow][sch + 8]) = kreg[1];
    if (want_t) {
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          ksT[sch + c * 8 + 2 * e][tcol] = (bf16_t)(kreg[c][e] & 0xffffu);
          ksT[sch + c * 8 + 2 * e + 1][tcol] = (bf16_t)(kreg[c][e] >> 16);
        }
    }
    if (want_v) {
      *reinterpret_cast<u32x4*>(&vs[srow][sch]) = vreg[0];
      *reinterpret_cast<u32x4*>(&vs[srow][sch + 8]) = vreg[1];
    }
  };
  auto scores = [&](f32x4 (&sa)[4], f32x4 (&da)[4], bool want_d) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f32x4 sacc = {0.f, 0.f, 0.f, 0.f}, dacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&ks[t * 16 + l15][kk * 32 + l4 * 8]);
        sacc = mfma16b<F16>(qf[kk], kf, sacc);
        if (want_d) {
          const bf16x8 vf = *reinterpret_cast<const bf16x8*>(&vs[t * 16 + l15][kk * 32 + l4 * 8]);
          dacc = mfma16b<F16>(gf[kk], vf, dacc);
        }
      }
      sa[t] = sacc * scale;
      da[t] = dacc;
    }
  };
  // one sweep over the key blocks 0..qb: body(kb, S tiles, dP tiles) runs with block kb staged and block kb + 1 in flight
  auto sweep = [&](bool want_v, auto&& body) {
    fetch(0, want_v);
    for (int kb = 0; kb <= qb; ++kb) {
      __syncthreads();  // everyone is done with the previous block (and with the output tiles of the previous body)
      stage(want_v);
      __syncthreads();
      if (kb < qb) fetch(kb + 1, want_v);
      f32x4 sa[4], da[4];
      scores(sa, da, want_v);
      body(kb, sa, da);
    }
  };
  auto group16 = [&](float v, bool is_max) {  // reduce over the 16 lanes that share l >> 4 (one query row each e)
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const float w = __shfl_xor(v, o, 64);
      v = is_max ? fmaxf(v, w) : v + w;
    }
    return v;
  };
  // first sweep: row maximum, row sum and sum(P dP) in ONE pass -- every lane runs an online softmax over the keys it sees
  // (its own running maximum; sums rescaled when it moves), the 16 lanes of a row are merged afterwards
  float m[4] = {-1e30f, -1e30f, -1e30f, -1e30f};
  float sum[4] = {0.f, 0.f, 0.f, 0.f}, dot[4] = {0.f, 0.f, 0.f, 0.f};
  float inv[4];
  if (lse) {  // (uniform) statistics from the forward: no first sweep
    // dO . O of query row wave * 16 + l15: this lane's 16 elements of the A-fragment rows, then the four lane groups
    float dsum = 0.f;
    {
      const long ar = row0 + min(q0 + wave * 16 + l15, T - 1);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const u32x4 ov = *reinterpret_cast<const u32x4*>(att + ar * (long)(nq * 64) + h * 64 + kk * 32 + l4 * 8);
        const u32x4 gv = __builtin_bit_cast(u32x4, gf[kk]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          dsum = fmaf(from16_lo<F16>(ov[e]), from16_lo<F16>(gv[e]), dsum);
          dsum = fmaf(from16_hi<F16>(ov[e]), from16_hi<F16>(gv[e]), dsum);
        }
      }
    }
    dsum += __shfl_xor(dsum, 16, 64);
    dsum += __shfl_xor(dsum, 32, 64);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = q0 + wave * 16 + l4 * 4 + e;
      m[e] = lse[bh * T + min(i, T - 1)];
      inv[e] = 1.f;
      dot[e] = __shfl(dsum, l4 * 4 + e, 64);  // (lane l4 * 4 + e holds row l4 * 4 + e: its l15)
      if (stats && l15 == 0 && i < T) *reinterpret_cast<f32x4*>(stats + (bh * T + i) * 4) = f32x4{m[e], 1.f, dot[e], 0.f};
    }
  } else {
  sweep(true, [&](int kb, f32x4 (&sa)[4], f32x4 (&da)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float tm = m[e];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (kb * 64 + t * 16 + l15 < nv[e]) tm = fmaxf(tm, sa[t][e]);
      const float resc = __expf(m[e] - tm);  // 1 when the maximum did not move; 0 * 0 on the first valid key
      sum[e] *= resc;
      dot[e] *= resc;
      m[e] = tm;
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (kb * 64 + t * 16 + l15 < nv[e]) {
          const float ex = __expf(sa[t][e] - tm);
          sum[e] += ex;
          dot[e] = fmaf(ex, da[t][e], dot[e]);
        }
    }
  });
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float mr = group16(m[e], true);
    const float resc = __expf(m[e] - mr);
    sum[e] *= resc;
    dot[e] *= resc;
    m[e] = mr;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    sum[e] = group16(sum[e], false);
    dot[e] = group16(dot[e], false);
    inv[e] = sum[e] > 0.f ? 1.f / sum[e] : 0.f;
    dot[e] *= inv[e];
    const int i = q0 + wave * 16 + l4 * 4 + e;
    if (stats && l15 == 0 && i < T) *reinterpret_cast<f32x4*>(stats + (bh * T + i) * 4) = f32x4{m[e], inv[e], dot[e], 0.f};
  }
  }  // (two-sweep form)
  f32x4 dq[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  want_t = dQ != nullptr;
  sweep(true, [&](int kb, f32x4 (&sa)[4], f32x4 (&da)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int cl = t * 16 + l15;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pv = 0.f, dv = 0.f;
        if (kb * 64 + cl < nv[e]) {
          pv = __expf(sa[t][e] - m[e]) * inv[e];
          dv = scale * pv * (da[t][e] - dot[e]);
        }
        const int r = wave * 16 + l4 * 4 + e;
        tP[r][cl] = to16<F16>(pv);
        tD[r][cl] = to16<F16>(dv);
      }
    }
    __syncthreads();
    // 8-byte stores: one instruction covers 4 rows x 16 lanes x 4 elements (2-byte stores, one row per instruction, cost
    // 48 store instructions per wave and block; these are 12)
#pragma unroll
    for (int it = 0; it < 4; ++it) {  // dS row-major: query row r, key quad l15
      const int r = wave * 16 + it * 4 + l4, i = q0 + r;
      const unsigned int* src = reinterpret_cast<const unsigned int*>(&tD[r][l15 * 4]);
      const u32x2 v = {src[0], src[1]};
      if (dS && i < T) *reinterpret_cast<u32x2*>(dS + (bh * T + i) * Tp + kb * 64 + l15 * 4) = v;
    }
    if (dQ) {  // dQ[16 rows of this wave][64] += dS tile [16 x 64 keys] . K block [64 keys x 64]
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const unsigned int* ap = reinterpret_cast<const unsigned int*>(&tD[wave * 16 + l15][kk * 32 + l4 * 8]);
        const u32x4 av = {ap[0], ap[1], ap[2], ap[3]};
        const bf16x8 af = __builtin_bit_cast(bf16x8, av);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const bf16x8 bfr = *reinterpret_cast<const bf16x8*>(&ksT[dt * 16 + l15][((kk * 4 + l4) ^ dt) * 8]);
          dq[dt] = mfma16b<F16>(af, bfr, dq[dt]);
        }
      }
    }
#pragma unroll
    for (int it = 0; it < 4 && PT != nullptr; ++it) {  // transposed tiles: key row cc, query quad l15
      const int cc = wave * 16 + it * 4 + l4, qs = l15 * 4;
      const u32x2 pv = {(unsigned int)tP[qs][cc] | ((unsigned int)tP[qs + 1][cc] << 16),
                        (unsigned int)tP[qs + 2][cc] | ((unsigned int)tP[qs + 3][cc] << 16)};
      const u32x2 dv = {(unsigned int)tD[qs][cc] | ((unsigned int)tD[qs + 1][cc] << 16),
                        (unsigned int)tD[qs + 2][cc] | ((unsigned int)tD[qs + 3][cc] << 16)};
      const long o = (bh * Tp + kb * 64 + cc) * Tp + q0 + qs;
      *reinterpret_cast<u32x2*>(PT + o) = pv;
      *reinterpret_cast<u32x2*>(dST + o) = dv;
    }
    // (the sweep's barrier before the next stage() also covers these tile reads)
  });
  if (dQ) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = q0 + wave * 16 + l4 * 4 + e;
        if (i < T) dQ[(row0 + i) * ld_dq + h * 64 + dt * 16 + l15] = dq[dt][e];
      }
  }
}


// ---------------------------------------------------------------------------
// dQ of the attention backward from the forward's row statistics (the product form of the query-major half when the tape
// holds lse and the attention's output: T <= 256, 16 % (nq / nkv) == 0).  One workgroup per (sample, key/value head) as in
// the forward: K, V (row-major) and K^T of the head are staged in LDS ONCE -- 110 KB -- and sixteen waves walk
// (query head, strip of 16 queries) units with no barrier after the staging one; the strips are dealt in (short, long)
// pairs, so every wave sees the same number of keys.  attn_bwd_scores_kernel re-staged the K / V block for every query
// head and every block of 64 queries (two barriers each) and passed P and dS through LDS tiles with two-byte stores.
//   S^T = K q^T and dP^T = V dO^T  (keys x queries: A = K / V rows from LDS, B = the strip's q / dO rows in registers)
//   P = exp(s - lse),  dS = scale P (dP - dO . O)   per element; D[m][n] sits in lane l as key 4 (l >> 4) + e, query l & 15
//   dQ += dS K: the lane's eight values of two key tiles ARE its A fragment (contraction index = keys, taken in the order
//   tile 0 keys 4 g .. 4 g + 3, tile 1 keys 4 g .. 4 g + 3), the B fragment reads K^T with the same key order.
// Nothing is written but dQ (fp32, head h at columns 64 h) and stats = (lse, 1, dO . O, 0) for attn_bwd_dkv_kernel.
// ---------------------------------------------------------------------------
constexpr int ABQ_WAVES = 16;

// The gradient of 16 rows x 64 dimensions of one head in MFMA accumulator layout (acc[dt][e]: row r0 + 4 (l >> 4) + e,
// dimension 16 dt + (l & 15)) -> the 16-bit gradient of the projections' outputs: dimensions d and d + 32 of a row sit in
// the same lane (dt and dt + 2), so the transposed rotation of rope_bwd_pack_kernel needs no exchange:
//   g_t1 = g_o1 cos + g_o2 sin,   g_t2 = g_o2 cos - g_o1 sin     (position = row inside the sample)
template <bool F16>
__device__ __forceinline__ void store_grad16(const f32x4 (&acc)[4], bf16_t* __restrict__ out, long ld, long row0, int r0, int T,
                                             int col0, bool rotate, const float* __restrict__ cosT,
                                             const float* __restrict__ sinT, int lane) {
  const int l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = r0 + 4 * l4 + e;
    if (i >= T) continue;
    bf16_t* o = out + (row0 + i) * ld + col0 + l15;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      float a = acc[w][e], b2 = acc[w + 2][e];
      if (rotate) {
        const float cs = cosT[i * 32 + w * 16 + l15], sn = sinT[i * 32 + w * 16 + l15];
        const float t1 = a * cs + b2 * sn, t2 = b2 * cs - a * sn;
        a = t1;
        b2 = t2;
      }
      o[w * 16] = to16<F16>(a);
      o[w * 16 + 32] = to16<F16>(b2);
    }
  }
}

template <bool F16>
__global__ __launch_bounds__(ABQ_WAVES * 64) void attn_bwd_dq_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dO,
                                                                     const bf16_t* __restrict__ att, const float* __restrict__ lse,
                                                                     float* __restrict__ dQ, long ld_dq, float* __restrict__ stats,
                                                                     const int* __restrict__ kv_len, int T, int Tp, int nq, int nkv,
                                                                     float scale, bf16_t* __restrict__ g16,
                                                                     const float* __restrict__ cosT, const float* __restrict__ sinT) {
  // g16 (optional, with cosT / sinT [T][32]): the 16-bit gradient of the q|k|v projection's output [B*T][(nq + 2 nkv) * 64];
  // the q columns are written here directly, transposed rotation applied (then dQ is not written: no fp32 round trip and
  // no rope_bwd_pack launch)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* Ks = reinterpret_cast<bf16_t*>(smem);                 // [Tp][72]
  bf16_t* Vs = Ks + Tp * 72;                                    // [Tp][72]
  bf16_t* KT = Vs + Tp * 72;                                    // [64][Tp + 4]
  const int kts = Tp + 4;
  const int group = nq / nkv;
  const int b = blockIdx.x / nkv, j = blockIdx.x % nkv;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const long nqkv = (long)(nq + 2 * nkv) * 64;
  const long row0 = (long)b * T;
  const int klen = min(kv_len[b], T);
  // ---- stage K, V, K^T: thread (key pair kp, 16-byte chunk c): rows 2 kp, 2 kp + 1; all loads first, rows >= T as zeros
  {
    const bf16_t* kbase = qkv + (nq + j) * 64;
    const bf16_t* vbase = qkv + (nq + nkv + j) * 64;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    for (int idx = threadIdx.x; idx < (Tp >> 1) * 8; idx += ABQ_WAVES * 64) {
      const int kp = idx >> 3, c = idx & 7;
      const int r0 = 2 * kp, r1 = r0 + 1;
      const long g0 = (row0 + min(r0, T - 1)) * nqkv + c * 8, g1 = (row0 + min(r1, T - 1)) * nqkv + c * 8;
      u32x4 ka = *reinterpret_cast<const u32x4*>(kbase + g0), kb = *reinterpret_cast<const u32x4*>(kbase + g1);
      u32x4 va = *reinterpret_cast<const u32x4*>(vbase + g0), vb = *reinterpret_cast<const u32x4*>(vbase + g1);
      if (r0 >= T) { ka = zero4; va = zero4; }
      if (r1 >= T) { kb = zero4; vb = zero4; }
      *reinterpret_cast<u32x4*>(Ks + r0 * 72 + c * 8) = ka;
      *reinterpret_cast<u32x4*>(Ks + r1 * 72 + c * 8) = kb;
      *reinterpret_cast<u32x4*>(Vs + r0 * 72 + c * 8) = va;
      *reinterpret_cast<u32x4*>(Vs + r1 * 72 + c * 8) = vb;
#pragma unroll
      for (int e = 0; e < 4; ++e) {  // two keys of one dimension per dword
        *reinterpret_cast<unsigned int*>(KT + (c * 8 + 2 * e) * kts + r0) = (ka[e] & 0xffffu) | (kb[e] << 16);
        *reinterpret_cast<unsigned int*>(KT + (c * 8 + 2 * e + 1) * kts + r0) = (ka[e] >> 16) | (kb[e] & 0xffff0000u);
      }
    }
  }
  __syncthreads();
  // ---- units: wave w serves query head w % group; its strips come in pairs (k, nstrips - 1 - k), k = w / group + NG * i
  const int h = j * group + wave % group;
  const int g0w = wave / group, NG = ABQ_WAVES / group;
  const int nstrips = (T + 15) >> 4;
  const int npair = (nstrips + 1) >> 1;
  const float c2 = scale * 1.4426950408889634f;
  for (int u = 0;; ++u) {
    const int pr = g0w + NG * (u >> 1);
    if (pr >= npair) break;  // (uniform)
    const int strip = (u & 1) ? nstrips - 1 - pr : pr;
    if ((u & 1) && strip == pr) continue;  // odd count: the middle strip is its own pair
    const int qi = strip * 16 + l15;       // this lane's query (B-fragment column / D column)
    const long ar = row0 + min(qi, T - 1);
    bf16x8 qf[2], gf[2];
    float delta = 0.f;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      qf[kk] = *reinterpret_cast<const bf16x8*>(qkv + ar * nqkv + h * 64 + kk * 32 + l4 * 8);
      gf[kk] = *reinterpret_cast<const bf16x8*>(dO + ar * (long)(nq * 64) + h * 64 + kk * 32 + l4 * 8);
      const u32x4 ov = *reinterpret_cast<const u32x4*>(att + ar * (long)(nq * 64) + h * 64 + kk * 32 + l4 * 8);
      const u32x4 gv = __builtin_bit_cast(u32x4, gf[kk]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        delta = fmaf(from16_lo<F16>(ov[e]), from16_lo<F16>(gv[e]), delta);
        delta = fmaf(from16_hi<F16>(ov[e]), from16_hi<F16>(gv[e]), delta);
      }
    }
    delta += __shfl_xor(delta, 16, 64);
    delta += __shfl_xor(delta, 32, 64);
    const long srow = ((long)b * nq + h) * T + min(qi, T - 1);
    const float l_nat = lse[srow];
    const float l2 = l_nat * 1.4426950408889634f;
    const int nv = qi < T ? min(qi + 1, klen) : 0;
    if (stats && l4 == 0 && qi < T) *reinterpret_cast<f32x4*>(stats + srow * 4) = f32x4{l_nat, 1.f, delta, 0.f};
    f32x4 dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nkeys = min(strip * 16 + 16, klen);  // keys any query of the strip attends
    for (int k0 = 0; k0 < nkeys; k0 += 32) {
      f32x4 sa[2], da[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 sacc = {0.f, 0.f, 0.f, 0.f}, dacc = {0.f, 0.f, 0.f, 0.f};
        const int krow = k0 + t * 16 + l15;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + krow * 72 + kk * 32 + l4 * 8);
          const bf16x8 vf = *reinterpret_cast<const bf16x8*>(Vs + krow * 72 + kk * 32 + l4 * 8);
          sacc = mfma16b<F16>(kf, qf[kk], sacc);
          dacc = mfma16b<F16>(vf, gf[kk], dacc);
        }
        sa[t] = sacc;
        da[t] = dacc;
      }
      u32x4 af;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float ds[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int key = k0 + t * 16 + 4 * l4 + e;
          const float pv = key < nv ? __builtin_amdgcn_exp2f(fmaf(sa[t][e], c2, -l2)) : 0.f;
          ds[e] = scale * pv * (da[t][e] - delta);
        }
        af[2 * t] = pack16x2<F16>(ds[0], ds[1]);
        af[2 * t + 1] = pack16x2<F16>(ds[2], ds[3]);
      }
      const bf16x8 afr = __builtin_bit_cast(bf16x8, af);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16_t* kt = KT + (dt * 16 + l15) * kts + k0 + 4 * l4;
        const u32x2 b0 = *reinterpret_cast<const u32x2*>(kt), b1 = *reinterpret_cast<const u32x2*>(kt + 16);
        const u32x4 bv = {b0[0], b0[1], b1[0], b1[1]};
        dq[dt] = mfma16b<F16>(afr, __builtin_bit_cast(bf16x8, bv), dq[dt]);
      }
    }
    if (g16) {
      store_grad16<F16>(dq, g16, nqkv, row0, strip * 16, T, h * 64, true, cosT, sinT, lane);
      continue;
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = strip * 16 + l4 * 4 + e;
        if (i < T) dQ[(row0 + i) * ld_dq + h * 64 + dt * 16 + l15] = dq[dt][e];
      }
  }
}
// bytes of its LDS image (Ks, Vs, KT above); attn_bwd_dq_long_kernel's is the same at Tp = ABL_CHUNK.  Limit set: 120 KiB
constexpr int attn_bwd_dq_lds(int Tp) { return (2 * Tp * 72 + 64 * (Tp + 4)) * 2; }
static_assert(attn_bwd_dq_lds(256) == 107008, "attn_bwd_dq_kernel: LDS image at Tp = 256");
static_assert(attn_bwd_dq_lds(256) <= 120 * 1024, "attn_bwd_dq_kernel: LDS image above the limit its entries set");

// ---------------------------------------------------------------------------
// dK, dV of the attention backward, key-major: one workgroup per (sample, key/value head, block of 64 keys); wave w owns
// 16 keys, whose K and V rows are its A fragments for the whole kernel.  For every query head of the group and every
// query block at or below the diagonal, the Q and dO blocks are staged in LDS (row-major for the score products,
// transposed for the gradient products), the tiles  S^T = K q^T  and  dP^T = V dO^T  are rebuilt on the matrix cores,
// P^T and dS^T follow from the per-query statistics attn_bwd_scores_kernel left behind, pass through a wave-private LDS
// tile (accumulator layout -> A-fragment layout), and  dV += P^T dO,  dK += dS^T q  accumulate in registers over all of
// it -- the group sum included.  Written once, fp32, into the k / v columns of the q|k|v-layout gradient.
// ---------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(256, 3) void attn_bwd_dkv_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dO,
                                                           const float* __restrict__ stats, float* __restrict__ g32,
                                                           const int* __restrict__ kv_len, int T, int Tp, int nq, int nkv,
                                                           float scale) {
  // (tP / tD, the P^T / dS^T tiles, reuse the storage of the row-major Q / dO blocks: one more barrier per iteration, 37 KB
  //  instead of 55 KB of LDS, three workgroups per CU instead of two)
  __shared__ __attribute__((aligned(16))) bf16_t qs[64][72], gs[64][72], qsT[64][72], gsT[64][72];
  bf16_t (*tP)[72] = qs;
  bf16_t (*tD)[72] = gs;
  __shared__ float st_m[64], st_inv[64], st_dot[64];
  __shared__ int st_nv[64];
  const int nkb = Tp >> 6;
  const int kb = blockIdx.x % nkb;
  const int bj = blockIdx.x / nkb;
  const int b = bj / nkv, j = bj % nkv;
  const int grp = nq / nkv;
  const int klen = min(kv_len[b], T);
  const int k0 = kb * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const long nqkv = (long)(nq + 2 * nkv) * 64;
  const long row0 = (long)b * T;
  bf16x8 kf[2], vf[2];
  {
    const long ar = row0 + min(k0 + wave * 16 + l15, T - 1);  // keys >= T: clamped load; they are >= nv of every query
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      kf[kk] = *reinterpret_cast<const bf16x8*>(qkv + ar * nqkv + (nq + j) * 64 + kk * 32 + l4 * 8);
      vf[kk] = *reinterpret_cast<const bf16x8*>(qkv + ar * nqkv + (nq + nkv + j) * 64 + kk * 32 + l4 * 8);
    }
  }
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dk[dt] = dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int srow = threadIdx.x >> 2, sch = (threadIdx.x & 3) * 16;
  const int tcol = (((srow >> 3) ^ (threadIdx.x & 3)) << 3) | (srow & 7);  // XOR-swizzled column of the transposed copies
  const int nit = grp * (nkb - kb);
  u32x4 qreg[2], greg[2];
  auto fetch = [&](int it) {
    const int h = j * grp + it / (nkb - kb), qb = kb + it % (nkb - kb);
    const long qr = row0 + min(qb * 64 + srow, T - 1);
    qreg[0] = *reinterpret_cast<const u32x4*>(qkv + qr * nqkv + h * 64 + sch);
    qreg[1] = *reinterpret_cast<const u32x4*>(qkv + qr * nqkv + h * 64 + sch + 8);
    greg[0] = *reinterpret_cast<const u32x4*>(dO + qr * (long)(nq * 64) + h * 64 + sch);
    greg[1] = *reinterpret_cast<const u32x4*>(dO + qr * (long)(nq * 64) + h * 64 + sch + 8);
  };
  fetch(0);
  for (int it = 0; it < nit; ++it) {
    const int h = j * grp + it / (nkb - kb), qb = kb + it % (nkb - kb);
    const int q0 = qb * 64;
    __syncthreads();  // the previous iteration is done with the staged blocks and the tiles
    *reinterpret_cast<u32x4*>(&qs[srow][sch]) = qreg[0];
    *reinterpret_cast<u32x4*>(&qs[srow][sch + 8]) = qreg[1];
    *reinterpret_cast<u32x4*>(&gs[srow][sch]) = greg[0];
    *reinterpret_cast<u32x4*>(&gs[srow][sch + 8]) = greg[1];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        qsT[sch + c * 8 + 2 * e][tcol] = (bf16_t)(qreg[c][e] & 0xffffu);
        qsT[sch + c * 8 + 2 * e + 1][tcol] = (bf16_t)(qreg[c][e] >> 16);
        gsT[sch + c * 8 + 2 * e][tcol] = (bf16_t)(greg[c][e] & 0xffffu);
        gsT[sch + c * 8 + 2 * e + 1][tcol] = (bf16_t)(greg[c][e] >> 16);
      }
    if (threadIdx.x < 64) {
      const int i = q0 + threadIdx.x;
      float m = 0.f, inv = 0.f, dot = 0.f;
      int nv = 0;
      if (i < T) {
        const f32x4 st = *reinterpret_cast<const f32x4*>(stats + (((long)b * nq + h) * T + i) * 4);
        m = st[0]; inv = st[1]; dot = st[2];
        nv = min(i + 1, klen);
      }
      st_m[threadIdx.x] = m; st_inv[threadIdx.x] = inv; st_dot[threadIdx.x] = dot; st_nv[threadIdx.x] = nv;
    }
    __syncthreads();
    if (it + 1 < nit) fetch(it + 1);
    f32x4 sT[4], dT[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {  // 16 keys of this wave x 16 queries
      f32x4 sacc = {0.f, 0.f, 0.f, 0.f}, dacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const bf16x8 qf = *reinterpret_cast<const bf16x8*>(&qs[t * 16 + l15][kk * 32 + l4 * 8]);
        const bf16x8 gf = *reinterpret_cast<const bf16x8*>(&gs[t * 16 + l15][kk * 32 + l4 * 8]);
        sacc = mfma16b<F16>(kf[kk], qf, sacc);
        dacc = mfma16b<F16>(vf[kk], gf, dacc);
      }
      sT[t] = sacc;
      dT[t] = dacc;
    }
    __syncthreads();  // every wave has read the row-major Q / dO blocks: their storage becomes the P^T / dS^T tiles
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 sacc = sT[t], dacc = dT[t];
      const int qi = t * 16 + l15;  // D[m][n]: m = key 4 l4 + e of the wave's 16, n = query qi
      const float qm = st_m[qi], qinv = st_inv[qi], qdot = st_dot[qi];
      const int qnv = st_nv[qi];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pv = 0.f, dsv = 0.f;
        if (k0 + wave * 16 + l4 * 4 + e < qnv) {
          pv = __expf(sacc[e] * scale - qm) * qinv;
          dsv = scale * pv * (dacc[e] - qdot);
        }
        tP[wave * 16 + l4 * 4 + e][qi] = to16<F16>(pv);
        tD[wave * 16 + l4 * 4 + e][qi] = to16<F16>(dsv);
      }
    }
    __syncthreads();  // (the tile rows of a wave are private to it; the barrier only orders its own writes and reads)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {  // contraction over the 64 queries of the block
      const bf16x8 pf = *reinterpret_cast<const bf16x8*>(&tP[wave * 16 + l15][kk * 32 + l4 * 8]);
      const bf16x8 df = *reinterpret_cast<const bf16x8*>(&tD[wave * 16 + l15][kk * 32 + l4 * 8]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16x8 gT = *reinterpret_cast<const bf16x8*>(&gsT[dt * 16 + l15][((kk * 4 + l4) ^ dt) * 8]);
        const bf16x8 qT = *reinterpret_cast<const bf16x8*>(&qsT[dt * 16 + l15][((kk * 4 + l4) ^ dt) * 8]);
        dv[dt] = mfma16b<F16>(pf, gT, dv[dt]);
        dk[dt] = mfma16b<F16>(df, qT, dk[dt]);
      }
    }
  }
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int key = k0 + wave * 16 + l4 * 4 + e;
      if (key < T) {
        g32[(row0 + key) * nqkv + (nq + j) * 64 + dt * 16 + l15] = dk[dt][e];
        g32[(row0 + key) * nqkv + (nq + nkv + j) * 64 + dt * 16 + l15] = dv[dt][e];
      }
    }
}

// ---------------------------------------------------------------------------
// dK, dV with the query side resident (T <= 256): one workgroup per (sample, key/value head), sixteen waves of 16 keys each
// (their K / V rows are B fragments held in registers for the whole kernel).  Per query head of the group, q and dO of ALL
// queries are staged once -- row-major for the score products, transposed (two queries per dword) for the gradient
// products: 140 KB -- and every wave walks the queries at or below its keys' diagonal, 32 at a time, without a barrier:
//   S = q K^T, dP = dO V^T as [queries x keys] tiles (A = q / dO rows from LDS): D[m][n] = query 4 (l >> 4) + e, key l & 15
//   P = exp(s - m) inv,  dS = scale P (dP - dot)         (statistics of the query, from LDS)
//   dV += P^T dO, dK += dS^T q: the lane's eight values of two query tiles ARE its A fragment (rows = keys, contraction
//   over queries in the order tile 0 queries 4 g .. 4 g + 3, tile 1 the same), B = dO^T / q^T read with the same order.
// attn_bwd_dkv_kernel re-staged a 64-query
// block per iteration behind four barriers and moved P^T / dS^T through LDS tiles with two-byte stores.
// ---------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(1024) void attn_bwd_dkv_res_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dO,
                                                                const float* __restrict__ stats, float* __restrict__ g32,
                                                                const int* __restrict__ kv_len, int T, int Tp, int nq, int nkv,
                                                                float scale, bf16_t* __restrict__ g16,
                                                                const float* __restrict__ cosT, const float* __restrict__ sinT) {
  // g16 (optional): as in attn_bwd_dq_kernel -- the k (rotation undone) and v columns go out as 16 bits, g32 is not written
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tts = Tp + 4;
  bf16_t* Qs = reinterpret_cast<bf16_t*>(smem);  // [Tp][72]
  bf16_t* Gs = Qs + Tp * 72;                     // [Tp][72]
  bf16_t* QT = Gs + Tp * 72;                     // [64][Tp + 4]
  bf16_t* GT = QT + 64 * tts;                    // [64][Tp + 4]
  float* st = reinterpret_cast<float*>(GT + 64 * tts);  // [3][Tp]: m * log2(e), 1 / sum, sum(P dP)
  const int grp = nq / nkv;
  const int b = blockIdx.x / nkv, j = blockIdx.x % nkv;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const long nqkv = (long)(nq + 2 * nkv) * 64;
  const long row0 = (long)b * T;
  const int klen = min(kv_len[b], T);
  // key strip of this wave: (s, 7 - s, 8 + s, 15 - s) for the four waves of SIMD s -- equal numbers of query tiles per SIMD
  const int sd = wave & 3, rr = wave >> 2;
  const int strip = rr == 0 ? sd : rr == 1 ? 7 - sd : rr == 2 ? 8 + sd : 15 - sd;
  const int key0 = strip * 16;
  const bool active = key0 < Tp;  // (uniform)
  bf16x8 kf[2], vf[2];
  {
    const long ar = row0 + min(key0 + l15, T - 1);  // keys >= T: clamped load; masked (>= klen)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      kf[kk] = *reinterpret_cast<const bf16x8*>(qkv + ar * nqkv + (nq + j) * 64 + kk * 32 + l4 * 8);
      vf[kk] = *reinterpret_cast<const bf16x8*>(qkv + ar * nqkv + (nq + nkv + j) * 64 + kk * 32 + l4 * 8);
    }
  }
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dk[dt] = dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  // staging: thread (query pair qp, 16-byte chunk c) -> rows 2 qp, 2 qp + 1 of q and dO (Tp / 2 * 8 <= 1024 pair-chunks)
  const int qp = threadIdx.x >> 3, ch = threadIdx.x & 7;
  const bool stager = threadIdx.x < (Tp >> 1) * 8;
  u32x4 qa, qb, ga, gb;
  auto fetch = [&](int hh) {
    const int h = j * grp + hh;
    const long g0 = row0 + min(2 * qp, T - 1), g1 = row0 + min(2 * qp + 1, T - 1);
    qa = *reinterpret_cast<const u32x4*>(qkv + g0 * nqkv + h * 64 + ch * 8);
    qb = *reinterpret_cast<const u32x4*>(qkv + g1 * nqkv + h * 64 + ch * 8);
    ga = *reinterpret_cast<const u32x4*>(dO + g0 * (long)(nq * 64) + h * 64 + ch * 8);
    gb = *reinterpret_cast<const u32x4*>(dO + g1 * (long)(nq * 64) + h * 64 + ch * 8);
  };
  const float c2 = scale * 1.4426950408889634f;
  for (int hh = 0; hh < grp; ++hh) {
    const int h = j * grp + hh;
    if (hh > 0) __syncthreads();  // everyone is done with the previous head's blocks
    // (keeping the next head's rows in flight in registers over this head's arithmetic pushed the kernel past its 128
    //  registers: measured slower, 40.5 vs 40.2 ms per step)
    if (stager) fetch(hh);
    if (stager) {
      const int r0 = 2 * qp, r1 = r0 + 1;
      const u32x4 zero4 = {0u, 0u, 0u, 0u};
      if (r0 >= T) { qa = zero4; ga = zero4; }
      if (r1 >= T) { qb = zero4; gb = zero4; }
      *reinterpret_cast<u32x4*>(Qs + r0 * 72 + ch * 8) = qa;
      *reinterpret_cast<u32x4*>(Qs + r1 * 72 + ch * 8) = qb;
      *reinterpret_cast<u32x4*>(Gs + r0 * 72 + ch * 8) = ga;
      *reinterpret_cast<u32x4*>(Gs + r1 * 72 + ch * 8) = gb;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        *reinterpret_cast<unsigned int*>(QT + (ch * 8 + 2 * e) * tts + r0) = (qa[e] & 0xffffu) | (qb[e] << 16);
        *reinterpret_cast<unsigned int*>(QT + (ch * 8 + 2 * e + 1) * tts + r0) = (qa[e] >> 16) | (qb[e] & 0xffff0000u);
        *reinterpret_cast<unsigned int*>(GT + (ch * 8 + 2 * e) * tts + r0) = (ga[e] & 0xffffu) | (gb[e] << 16);
        *reinterpret_cast<unsigned int*>(GT + (ch * 8 + 2 * e + 1) * tts + r0) = (ga[e] >> 16) | (gb[e] & 0xffff0000u);
      }
    }
    if ((int)threadIdx.x < Tp) {
      const int i = threadIdx.x;
      f32x4 sv = {0.f, 0.f, 0.f, 0.f};
      if (i < T) sv = *reinterpret_cast<const f32x4*>(stats + (((long)b * nq + h) * T + i) * 4);
      st[i] = sv[0] * 1.4426950408889634f;
      st[Tp + i] = i < T ? sv[1] : 0.f;  // (queries >= T: P = 0)
      st[2 * Tp + i] = sv[2];
    }
    __syncthreads();
    if (active) {
      for (int q0 = key0 & ~31; q0 < Tp; q0 += 32) {  // queries at or below the diagonal of this wave's keys
        f32x4 sa[2], da[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          f32x4 sacc = {0.f, 0.f, 0.f, 0.f}, dacc = {0.f, 0.f, 0.f, 0.f};
          const int qrow = q0 + t * 16 + l15;
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            const bf16x8 qf = *reinterpret_cast<const bf16x8*>(Qs + qrow * 72 + kk * 32 + l4 * 8);
            const bf16x8 gf = *reinterpret_cast<const bf16x8*>(Gs + qrow * 72 + kk * 32 + l4 * 8);
            sacc = mfma16b<F16>(qf, kf[kk], sacc);
            dacc = mfma16b<F16>(gf, vf[kk], dacc);
          }
          sa[t] = sacc;
          da[t] = dacc;
        }
        u32x4 pfr, dfr;
        const int key = key0 + l15;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int qi = q0 + t * 16 + 4 * l4;
          const f32x4 m2 = *reinterpret_cast<const f32x4*>(st + qi), iv = *reinterpret_cast<const f32x4*>(st + Tp + qi),
                      dt_ = *reinterpret_cast<const f32x4*>(st + 2 * Tp + qi);
          float pv[4], ds[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool ok = key <= qi + e && key < klen;  // (queries >= T have 1 / sum = 0)
            pv[e] = ok ? __builtin_amdgcn_exp2f(fmaf(sa[t][e], c2, -m2[e])) * iv[e] : 0.f;
            ds[e] = scale * pv[e] * (da[t][e] - dt_[e]);
          }
          pfr[2 * t] = pack16x2<F16>(pv[0], pv[1]);
          pfr[2 * t + 1] = pack16x2<F16>(pv[2], pv[3]);
          dfr[2 * t] = pack16x2<F16>(ds[0], ds[1]);
          dfr[2 * t + 1] = pack16x2<F16>(ds[2], ds[3]);
        }
        const bf16x8 pf = __builtin_bit_cast(bf16x8, pfr), df = __builtin_bit_cast(bf16x8, dfr);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const bf16_t* gt = GT + (dt * 16 + l15) * tts + q0 + 4 * l4;
          const bf16_t* qt = QT + (dt * 16 + l15) * tts + q0 + 4 * l4;
          const u32x2 g0 = *reinterpret_cast<const u32x2*>(gt), g1 = *reinterpret_cast<const u32x2*>(gt + 16);
          const u32x2 q0v = *reinterpret_cast<const u32x2*>(qt), q1v = *reinterpret_cast<const u32x2*>(qt + 16);
          const u32x4 gv = {g0[0], g0[1], g1[0], g1[1]}, qv = {q0v[0], q0v[1], q1v[0], q1v[1]};
          dv[dt] = mfma16b<F16>(pf, __builtin_bit_cast(bf16x8, gv), dv[dt]);
          dk[dt] = mfma16b<F16>(df, __builtin_bit_cast(bf16x8, qv), dk[dt]);
        }
      }
    }
  }
  if (!active) return;
  if (g16) {
    store_grad16<F16>(dk, g16, nqkv, row0, key0, T, (nq + j) * 64, true, cosT, sinT, lane);
    store_grad16<F16>(dv, g16, nqkv, row0, key0, T, (nq + nkv + j) * 64, false, cosT, sinT, lane);
    return;
  }
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int key = key0 + l4 * 4 + e;
      if (key < T) {
        g32[(row0 + key) * nqkv + (nq + j) * 64 + dt * 16 + l15] = dk[dt][e];
        g32[(row0 + key) * nqkv + (nq + nkv + j) * 64 + dt * 16 + l15] = dv[dt][e];
      }
    }
}
// bytes of its LDS image (Qs, Gs, QT, GT, st above); attn_bwd_dkv_long_kernel's is the same at Tp = ABL_CHUNK.  Limit set: 150 KiB
constexpr int attn_bwd_dkv_res_lds(int Tp) { return (2 * Tp * 72 + 2 * 64 * (Tp + 4)) * 2 + 3 * Tp * 4; }
static_assert(attn_bwd_dkv_res_lds(256) == 143360, "attn_bwd_dkv_res_kernel: LDS image at Tp = 256");
static_assert(attn_bwd_dkv_res_lds(256) <= 150 * 1024, "attn_bwd_dkv_res_kernel: LDS image above the limit its entries set");

// ---------------------------------------------------------------------------
// The two resident kernels above in chunks of 256, for 256 < T <= 544 (tcavt_attn_bwd_long; any T <= 544 is computed
// correctly).  The LDS images are those of ONE chunk, so a workgroup stays below 160 KB whatever T is.
//
// dQ: a workgroup owns (sample, key/value head, chunk of QC queries) and walks the key chunks 0 .. its own; K, V and K^T
// of a key chunk are staged behind a barrier pair (107 KB).  A wave keeps the dQ accumulators of its U (query head, strip)
// units in registers across the key chunks; q, dO, lse and dO . O of a unit are re-read per chunk (L2 hits) so that only the
// accumulators stay live.  U = min(group, 2) and QC = 256 U / group: 16 U units of 16 queries per workgroup, U per wave,
// whatever the group is (group 4 -> chunks of 128 queries, group 8 -> 64, group 16 -> 32; U = 4 at group 4 needed more
// than the 128 registers a wave of a 1024-thread workgroup has and spilled).  Strips are dealt in (short, long) pairs of
// the chunk as in the resident kernel: on the diagonal key chunk every wave sees the same number of keys.
// Workgroups of the LAST query chunks (most key chunks) come first in the grid.
// ---------------------------------------------------------------------------
constexpr int ABL_CHUNK = 256;
constexpr int ABL_KTS = ABL_CHUNK + 4;
constexpr int ABL_MAX_T = 544;

template <bool F16, int U>
__global__ __launch_bounds__(ABQ_WAVES * 64) void attn_bwd_dq_long_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dO,
                                                                          const bf16_t* __restrict__ att, const float* __restrict__ lse,
                                                                          float* __restrict__ stats, const int* __restrict__ kv_len,
                                                                          int T, int nq, int nkv, int nqc, int nbj, float scale,
                                                                          bf16_t* __restrict__ g16, const float* __restrict__ cosT,
                                                                          const float* __restrict__ sinT) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* Ks = reinterpret_cast<bf16_t*>(smem);  // [256][72]
  bf16_t* Vs = Ks + ABL_CHUNK * 72;              // [256][72]
  bf16_t* KT = Vs + ABL_CHUNK * 72;              // [64][260]
  const int group = nq / nkv;
  const int QC = ABL_CHUNK * U / group, nS = QC >> 4, NG = ABQ_WAVES / group;
  const int bj = blockIdx.x % nbj, qc = nqc - 1 - blockIdx.x / nbj;
  const int b = bj / nkv, j = bj % nkv;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const long nqkv = (long)(nq + 2 * nkv) * 64;
  const long row0 = (long)b * T;
  const int klen = min(kv_len[b], T);
  const int q_lo = qc * QC, q_hi = min(T, q_lo + QC);
  const int nkeys_wg = min(q_hi, klen);  // keys any query of this chunk attends
  const int h = j * group + wave % group;
  const int g0w = wave / group;
  const float c2 = scale * 1.4426950408889634f;
  f32x4 dq[U][4];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[u][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16_t* kbase = qkv + (nq + j) * 64;
  const bf16_t* vbase = qkv + (nq + nkv + j) * 64;
  for (int c = 0; c == 0 || c * ABL_CHUNK < nkeys_wg; ++c) {  // (uniform; chunk 0 always: it writes stats)
    const int kb0 = c * ABL_CHUNK;
    if (c > 0) __syncthreads();  // everyone is done with the previous chunk
    {
      // thread (key pair kp, 16-byte chunk ch): local rows 2 kp, 2 kp + 1; rows >= T as zeros (their loads clamped)
      const int nrow = max(0, min(ABL_CHUNK, (nkeys_wg - kb0 + 31) & ~31));
      const u32x4 zero4 = {0u, 0u, 0u, 0u};
      for (int idx = threadIdx.x; idx < (nrow >> 1) * 8; idx += ABQ_WAVES * 64) {
        const int kp = idx >> 3, ch = idx & 7;
        const int r0 = 2 * kp, r1 = r0 + 1;
        const long g0 = (row0 + min(kb0 + r0, T - 1)) * nqkv + ch * 8, g1 = (row0 + min(kb0 + r1, T - 1)) * nqkv + ch * 8;
        u32x4 ka = *reinterpret_cast<const u32x4*>(kbase + g0), kb = *reinterpret_cast<const u32x4*>(kbase + g1);
        u32x4 va = *reinterpret_cast<const u32x4*>(vbase + g0), vb = *reinterpret_cast<const u32x4*>(vbase + g1);
        if (kb0 + r0 >= T) { ka = zero4; va = zero4; }
        if (kb0 + r1 >= T) { kb = zero4; vb = zero4; }
        *reinterpret_cast<u32x4*>(Ks + r0 * 72 + ch * 8) = ka;
        *reinterpret_cast<u32x4*>(Ks + r1 * 72 + ch * 8) = kb;
        *reinterpret_cast<u32x4*>(Vs + r0 * 72 + ch * 8) = va;
        *reinterpret_cast<u32x4*>(Vs + r1 * 72 + ch * 8) = vb;
#pragma unroll
        for (int e = 0; e < 4; ++e) {  // two keys of one dimension per dword
          *reinterpret_cast<unsigned int*>(KT + (ch * 8 + 2 * e) * ABL_KTS + r0) = (ka[e] & 0xffffu) | (kb[e] << 16);
          *reinterpret_cast<unsigned int*>(KT + (ch * 8 + 2 * e + 1) * ABL_KTS + r0) = (ka[e] >> 16) | (kb[e] & 0xffff0000u);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int pr = g0w + NG * (u >> 1);
      const int strip = U == 1 ? g0w : (u & 1) ? nS - 1 - pr : pr;
      const int s0 = q_lo + strip * 16;  // first query of the unit
      if (s0 >= T) continue;             // (uniform)
      const int nkl = min(ABL_CHUNK, min(s0 + 16, klen) - kb0);  // keys of this chunk any query of the strip attends
      if (c > 0 && nkl <= 0) continue;                           // (uniform)
      const int qi = s0 + l15;  // this lane's query (B-fragment column / D column)
      const long ar = row0 + min(qi, T - 1);
      bf16x8 qf[2], gf[2];
      float delta = 0.f;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        qf[kk] = *reinterpret_cast<const bf16x8*>(qkv + ar * nqkv + h * 64 + kk * 32 + l4 * 8);
        gf[kk] = *reinterpret_cast<const bf16x8*>(dO + ar * (long)(nq * 64) + h * 64 + kk * 32 + l4 * 8);
        const u32x4 ov = *reinterpret_cast<const u32x4*>(att + ar * (long)(nq * 64) + h * 64 + kk * 32 + l4 * 8);
        const u32x4 gv = __builtin_bit_cast(u32x4, gf[kk]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          delta = fmaf(from16_lo<F16>(ov[e]), from16_lo<F16>(gv[e]), delta);
          delta = fmaf(from16_hi<F16>(ov[e]), from16_hi<F16>(gv[e]), delta);
        }
      }
      delta += __shfl_xor(delta, 16, 64);
      delta += __shfl_xor(delta, 32, 64);
      const long srow = ((long)b * nq + h) * T + min(qi, T - 1);
      const float l_nat = lse[srow];
      const float l2 = l_nat * 1.4426950408889634f;
      const int nv = qi < T ? min(qi + 1, klen) : 0;
      if (c == 0 && l4 == 0 && qi < T) *reinterpret_cast<f32x4*>(stats + srow * 4) = f32x4{l_nat, 1.f, delta, 0.f};
      for (int k0 = 0; k0 < nkl; k0 += 32) {
        f32x4 sa[2], da[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          f32x4 sacc = {0.f, 0.f, 0.f, 0.f}, dacc = {0.f, 0.f, 0.f, 0.f};
          const int krow = k0 + t * 16 + l15;
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + krow * 72 + kk * 32 + l4 * 8);
            const bf16x8 vf = *reinterpret_cast<const bf16x8*>(Vs + krow * 72 + kk * 32 + l4 * 8);
            sacc = mfma16b<F16>(kf, qf[kk], sacc);
            dacc = mfma16b<F16>(vf, gf[kk], dacc);
          }
          sa[t] = sacc;
          da[t] = dacc;
        }
        u32x4 af;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          float ds[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int key = kb0 + k0 + t * 16 + 4 * l4 + e;
            const float pv = key < nv ? __builtin_amdgcn_exp2f(fmaf(sa[t][e], c2, -l2)) : 0.f;
            ds[e] = scale * pv * (da[t][e] - delta);
          }
          af[2 * t] = pack16x2<F16>(ds[0], ds[1]);
          af[2 * t + 1] = pack16x2<F16>(ds[2], ds[3]);
        }
        const bf16x8 afr = __builtin_bit_cast(bf16x8, af);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const bf16_t* kt = KT + (dt * 16 + l15) * ABL_KTS + k0 + 4 * l4;
          const u32x2 b0 = *reinterpret_cast<const u32x2*>(kt), b1 = *reinterpret_cast<const u32x2*>(kt + 16);
          const u32x4 bv = {b0[0], b0[1], b1[0], b1[1]};
          dq[u][dt] = mfma16b<F16>(afr, __builtin_bit_cast(bf16x8, bv), dq[u][dt]);
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int pr = g0w + NG * (u >> 1);
    const int strip = U == 1 ? g0w : (u & 1) ? nS - 1 - pr : pr;
    const int s0 = q_lo + strip * 16;
    if (s0 < T) store_grad16<F16>(dq[u], g16, nqkv, row0, s0, T, h * 64, true, cosT, sinT, lane);
  }
}

// dK, dV: a workgroup owns (sample, key/value head, chunk of 256 keys), sixteen waves of 16 keys (K / V rows in registers,
// dK / dV accumulators in registers for the whole kernel, as in attn_bwd_dkv_res_kernel) and walks the query heads of the
// group and, per head, the query chunks from its own upward; q, dO, their transposes and the row statistics of a query
// chunk are staged behind a barrier pair (140 KB).  Workgroups of key chunk 0 (most query chunks) come first in the grid;
// a chunk that starts at or beyond kv_len writes its zeros and leaves.
template <bool F16>
__global__ __launch_bounds__(1024) void attn_bwd_dkv_long_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dO,
                                                                 const float* __restrict__ stats, const int* __restrict__ kv_len,
                                                                 int T, int nq, int nkv, int nbj, float scale,
                                                                 bf16_t* __restrict__ g16, const float* __restrict__ cosT,
                                                                 const float* __restrict__ sinT) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* Qs = reinterpret_cast<bf16_t*>(smem);  // [256][72]
  bf16_t* Gs = Qs + ABL_CHUNK * 72;              // [256][72]
  bf16_t* QT = Gs + ABL_CHUNK * 72;              // [64][260]
  bf16_t* GT = QT + 64 * ABL_KTS;                // [64][260]
  float* st = reinterpret_cast<float*>(GT + 64 * ABL_KTS);  // [3][256]: lse * log2(e), 1 / sum, dO . O
  const int Tp = (T + 63) & ~63;
  const int grp = nq / nkv;
  const int bj = blockIdx.x % nbj, kc = blockIdx.x / nbj;
  const int b = bj / nkv, j = bj % nkv;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const long nqkv = (long)(nq + 2 * nkv) * 64;
  const long row0 = (long)b * T;
  const int klen = min(kv_len[b], T);
  // key strip of this wave: (s, 7 - s, 8 + s, 15 - s) for the four waves of SIMD s -- equal numbers of query tiles per SIMD
  const int sd = wave & 3, rr = wave >> 2;
  const int strip = rr == 0 ? sd : rr == 1 ? 7 - sd : rr == 2 ? 8 + sd : 15 - sd;
  const int kl0 = strip * 16, key0 = kc * ABL_CHUNK + kl0;
  const bool active = key0 < T;            // (uniform) this wave has rows to write
  const bool work = key0 < klen;           // (uniform) ... and they are not all zero
  bf16x8 kf[2], vf[2];
  {
    const long ar = row0 + min(key0 + l15, T - 1);  // keys >= T: clamped load; masked (>= klen)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      kf[kk] = *reinterpret_cast<const bf16x8*>(qkv + ar * nqkv + (nq + j) * 64 + kk * 32 + l4 * 8);
      vf[kk] = *reinterpret_cast<const bf16x8*>(qkv + ar * nqkv + (nq + nkv + j) * 64 + kk * 32 + l4 * 8);
    }
  }
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dk[dt] = dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int qp = threadIdx.x >> 3, ch = threadIdx.x & 7;  // staging: query pair qp, 16-byte chunk ch
  const float c2 = scale * 1.4426950408889634f;
  const int nqc = kc * ABL_CHUNK < klen ? (Tp + ABL_CHUNK - 1) / ABL_CHUNK : kc;  // (uniform; no key < kv_len: no walk)
  bool first = true;
  for (int hh = 0; hh < grp; ++hh) {
    const int h = j * grp + hh;
    for (int qcx = kc; qcx < nqc; ++qcx) {
      const int qb0 = qcx * ABL_CHUNK;
      const int nrow = min(ABL_CHUNK, Tp - qb0);  // (a multiple of 64)
      if (!first) __syncthreads();                // everyone is done with the previous blocks
      first = false;
      if ((int)threadIdx.x < (nrow >> 1) * 8) {
        const int r0 = 2 * qp, r1 = r0 + 1;
        const long g0 = row0 + min(qb0 + r0, T - 1), g1 = row0 + min(qb0 + r1, T - 1);
        u32x4 qa = *reinterpret_cast<const u32x4*>(qkv + g0 * nqkv + h * 64 + ch * 8);
        u32x4 qb = *reinterpret_cast<const u32x4*>(qkv + g1 * nqkv + h * 64 + ch * 8);
        u32x4 ga = *reinterpret_cast<const u32x4*>(dO + g0 * (long)(nq * 64) + h * 64 + ch * 8);
        u32x4 gb = *reinterpret_cast<const u32x4*>(dO + g1 * (long)(nq * 64) + h * 64 + ch * 8);
        const u32x4 zero4 = {0u, 0u, 0u, 0u};
        if (qb0 + r0 >= T) { qa = zero4; ga = zero4; }
        if (qb0 + r1 >= T) { qb = zero4; gb = zero4; }
        *reinterpret_cast<u32x4*>(Qs + r0 * 72 + ch * 8) = qa;
        *reinterpret_cast<u32x4*>(Qs + r1 * 72 + ch * 8) = qb;
        *reinterpret_cast<u32x4*>(Gs + r0 * 72 + ch * 8) = ga;
        *reinterpret_cast<u32x4*>(Gs + r1 * 72 + ch * 8) = gb;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          *reinterpret_cast<unsigned int*>(QT + (ch * 8 + 2 * e) * ABL_KTS + r0) = (qa[e] & 0xffffu) | (qb[e] << 16);
          *reinterpret_cast<unsigned int*>(QT + (ch * 8 + 2 * e + 1) * ABL_KTS + r0) = (qa[e] >> 16) | (qb[e] & 0xffff0000u);
          *reinterpret_cast<unsigned int*>(GT + (ch * 8 + 2 * e) * ABL_KTS + r0) = (ga[e] & 0xffffu) | (gb[e] << 16);
          *reinterpret_cast<unsigned int*>(GT + (ch * 8 + 2 * e + 1) * ABL_KTS + r0) = (ga[e] >> 16) | (gb[e] & 0xffff0000u);
        }
      }
      if ((int)threadIdx.x < nrow) {
        const int il = threadIdx.x, i = qb0 + il;
        f32x4 sv = {0.f, 0.f, 0.f, 0.f};
        if (i < T) sv = *reinterpret_cast<const f32x4*>(stats + (((long)b * nq + h) * T + i) * 4);
        st[il] = sv[0] * 1.4426950408889634f;
        st[ABL_CHUNK + il] = i < T ? sv[1] : 0.f;  // (queries >= T: P = 0)
        st[2 * ABL_CHUNK + il] = sv[2];
      }
      __syncthreads();
      if (!work) continue;
      // queries at or below the diagonal of this wave's keys: the whole chunk when it lies below the key chunk
      for (int q0 = qcx == kc ? (kl0 & ~31) : 0; q0 < nrow; q0 += 32) {
        f32x4 sa[2], da[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          f32x4 sacc = {0.f, 0.f, 0.f, 0.f}, dacc = {0.f, 0.f, 0.f, 0.f};
          const int qrow = q0 + t * 16 + l15;
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            const bf16x8 qf = *reinterpret_cast<const bf16x8*>(Qs + qrow * 72 + kk * 32 + l4 * 8);
            const bf16x8 gf = *reinterpret_cast<const bf16x8*>(Gs + qrow * 72 + kk * 32 + l4 * 8);
            sacc = mfma16b<F16>(qf, kf[kk], sacc);
            dacc = mfma16b<F16>(gf, vf[kk], dacc);
          }
          sa[t] = sacc;
          da[t] = dacc;
        }
        u32x4 pfr, dfr;
        const int key = key0 + l15;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int ql = q0 + t * 16 + 4 * l4, qi = qb0 + ql;
          const f32x4 m2 = *reinterpret_cast<const f32x4*>(st + ql), iv = *reinterpret_cast<const f32x4*>(st + ABL_CHUNK + ql),
                      dt_ = *reinterpret_cast<const f32x4*>(st + 2 * ABL_CHUNK + ql);
          float pv[4], ds[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool ok = key <= qi + e && key < klen;  // (queries >= T have 1 / sum = 0)
            pv[e] = ok ? __builtin_amdgcn_exp2f(fmaf(sa[t][e], c2, -m2[e])) * iv[e] : 0.f;
            ds[e] = scale * pv[e] * (da[t][e] - dt_[e]);
          }
          pfr[2 * t] = pack16x2<F16>(pv[0], pv[1]);
          pfr[2 * t + 1] = pack16x2<F16>(pv[2], pv[3]);
          dfr[2 * t] = pack16x2<F16>(ds[0], ds[1]);
          dfr[2 * t + 1] = pack16x2<F16>(ds[2], ds[3]);
        }
        const bf16x8 pf = __builtin_bit_cast(bf16x8, pfr), df = __builtin_bit_cast(bf16x8, dfr);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const bf16_t* gt = GT + (dt * 16 + l15) * ABL_KTS + q0 + 4 * l4;
          const bf16_t* qt = QT + (dt * 16 + l15) * ABL_KTS + q0 + 4 * l4;
          const u32x2 g0 = *reinterpret_cast<const u32x2*>(gt), g1 = *reinterpret_cast<const u32x2*>(gt + 16);
          const u32x2 q0v = *reinterpret_cast<const u32x2*>(qt), q1v = *reinterpret_cast<const u32x2*>(qt + 16);
          const u32x4 gv = {g0[0], g0[1], g1[0], g1[1]}, qv = {q0v[0], q0v[1], q1v[0], q1v[1]};
          dv[dt] = mfma16b<F16>(pf, __builtin_bit_cast(bf16x8, gv), dv[dt]);
          dk[dt] = mfma16b<F16>(df, __builtin_bit_cast(bf16x8, qv), dk[dt]);
        }
      }
    }
  }
  if (!active) return;
  store_grad16<F16>(dk, g16, nqkv, row0, key0, T, (nq + j) * 64, true, cosT, sinT, lane);
  store_grad16<F16>(dv, g16, nqkv, row0, key0, T, (nq + nkv + j) * 64, false, cosT, sinT, lane);
}

}  // namespace tcavt

using namespace tcavt;

#define TCAVT_TRY(call)            \
  do {                             \
    const int rc_ = (call);        \
    if (rc_ != TCAVT_OK) return rc_; \
  } while (0)

extern "C" int tcavt_rope_bwd_pack(const float* g32, void* out_bf16, const float* rope_cos, const float* rope_sin, int64_t M,
                                   int ncols, int rope_cols, int L, int dtype16, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(is16(dtype16), "rope_bwd_pack: dtype16 must be TCAVT_BF16 or TCAVT_F16");
  TCAVT_CHECK_ARG(g32 && out_bf16 && rope_cos && rope_sin && M > 0 && L > 0, "rope_bwd_pack: bad args");
  TCAVT_CHECK_ARG(ncols % 64 == 0 && rope_cols % 64 == 0 && rope_cols <= ncols, "rope_bwd_pack: columns come in heads of 64");
  const long n = (long)M * (ncols / 2);
  auto kfn = dtype16 == TCAVT_F16 ? rope_bwd_pack_kernel<true> : rope_bwd_pack_kernel<false>;
  hipLaunchKernelGGL(kfn, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     g32, static_cast<bf16_t*>(out_bf16), rope_cos, rope_sin, (long)M, ncols, rope_cols, L);
  TCAVT_CHECK_LAUNCH("rope_bwd_pack");
  return TCAVT_OK;
}

// the query heads of a key/value head share the sixteen waves of a workgroup (resident and chunked kernels)
static bool group_ok(int nq, int nkv) { return nq > 0 && nkv > 0 && nq % nkv == 0 && ABQ_WAVES % (nq / nkv) == 0; }

// (A/B switch) tcavt_attn_bwd_scores / tcavt_attn_bwd_dkv keep to the tiled pair where they would take a resident kernel
static bool resident_off() {
  static const bool off = getenv("TCAVT_ATTN_BWD_NO_RESIDENT") != nullptr;
  return off;
}

// What the two resident kernels share of a call; one workgroup per (sample, key/value head) in both.
struct ResidentArgs {
  const void *qkv, *dO;
  const int32_t* kv_len;
  int B, T, Tp, nq, nkv;
  float scale;
  int dtype16;
  tcavt_stream_t stream;
};
// Each writes fp32 (dQ with its leading dimension / g32) or, with the RoPE tables, the 16-bit g16; the other output is null.
// `who` is the entry point in the attribute's message, `label` the launch in TCAVT_CHECK_LAUNCH's.
static int launch_dq(const ResidentArgs& a, const char* who, const char* label, const void* att, const float* lse, float* dQ,
                     long ld_dq, float* stats, void* g16, const float* rope_cos, const float* rope_sin) {
  const bool f16 = a.dtype16 == TCAVT_F16;
  auto kq = f16 ? attn_bwd_dq_kernel<true> : attn_bwd_dq_kernel<false>;
  static bool limit_set[2] = {false, false};
  TCAVT_TRY(dyn_lds_limit(reinterpret_cast<const void*>(kq), 120 * 1024, who, limit_set[f16]));
  hipLaunchKernelGGL(kq, dim3((unsigned)(a.B * a.nkv)), dim3(ABQ_WAVES * 64), attn_bwd_dq_lds(a.Tp), static_cast<hipStream_t>(a.stream),
                     static_cast<const bf16_t*>(a.qkv), static_cast<const bf16_t*>(a.dO), static_cast<const bf16_t*>(att), lse, dQ, ld_dq,
                     stats, a.kv_len, a.T, a.Tp, a.nq, a.nkv, a.scale, static_cast<bf16_t*>(g16), rope_cos, rope_sin);
  TCAVT_CHECK_LAUNCH(label);
  return TCAVT_OK;
}
static int launch_dkv_res(const ResidentArgs& a, const char* who, const char* label, const float* stats, float* g32, void* g16,
                          const float* rope_cos, const float* rope_sin) {
  const bool f16 = a.dtype16 == TCAVT_F16;
  auto kr = f16 ? attn_bwd_dkv_res_kernel<true> : attn_bwd_dkv_res_kernel<false>;
  static bool limit_set[2] = {false, false};
  TCAVT_TRY(dyn_lds_limit(reinterpret_cast<const void*>(kr), 150 * 1024, who, limit_set[f16]));
  hipLaunchKernelGGL(kr, dim3((unsigned)(a.B * a.nkv)), dim3(1024), attn_bwd_dkv_res_lds(a.Tp), static_cast<hipStream_t>(a.stream),
                     static_cast<const bf16_t*>(a.qkv), static_cast<const bf16_t*>(a.dO), stats, g32, a.kv_len, a.T,
                     a.Tp, a.nq, a.nkv, a.scale, static_cast<bf16_t*>(g16), rope_cos, rope_sin);
  TCAVT_CHECK_LAUNCH(label);
  return TCAVT_OK;
}

extern "C" int tcavt_attn_bwd_scores(const void* qkv_bf16, const void* dO_bf16, void* dS_bf16, void* PT_bf16, void* dST_bf16,
                                     float* dQ, int64_t ld_dq, float* stats, const int32_t* kv_len, int B, int T, int Tp,
                                     int nq, int nkv, int head_dim, float scale, int dtype16, const float* lse, const void* att,
                                     tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(qkv_bf16 && dO_bf16 && kv_len && B > 0 && T > 0 && is16(dtype16), "attn_bwd_scores: bad args");
  TCAVT_CHECK_ARG((lse != nullptr) == (att != nullptr) && aligned16(att), "attn_bwd_scores: lse and att come together (att 16-byte aligned)");
  TCAVT_CHECK_ARG((PT_bf16 != nullptr) == (dST_bf16 != nullptr), "attn_bwd_scores: PT and dST come together");
  TCAVT_CHECK_ARG(PT_bf16 || stats, "attn_bwd_scores: give PT/dST (GEMM form of dK, dV) or stats (tcavt_attn_bwd_dkv)");
  TCAVT_CHECK_ARG(aligned16(stats), "attn_bwd_scores: stats must be 16-byte aligned");
  TCAVT_CHECK_ARG(dS_bf16 || dQ, "attn_bwd_scores: give dQ (computed here) or dS (for an external dQ product), or both");
  TCAVT_CHECK_ARG(!dQ || ld_dq >= (int64_t)nq * 64, "attn_bwd_scores: ld_dq must cover nq * 64 columns");
  TCAVT_CHECK_ARG(head_dim == 64 && nkv > 0 && nq % nkv == 0, "attn_bwd_scores: head_dim 64 and nq %% nkv == 0 required");
  TCAVT_CHECK_ARG(Tp >= T && Tp - T < 64 && Tp % 64 == 0, "attn_bwd_scores: Tp must be T rounded up to a multiple of 64");
  TCAVT_CHECK_ARG(aligned16(qkv_bf16) && aligned16(dO_bf16), "attn_bwd_scores: 16-byte alignment required");
  if (lse && dQ && stats && !dS_bf16 && !PT_bf16 && Tp <= 256 && group_ok(nq, nkv) && !resident_off()) {
    // statistics from the forward, nothing but dQ wanted: K, V, K^T of a key/value head resident in LDS, no key-block loop
    const ResidentArgs r = {qkv_bf16, dO_bf16, kv_len, B, T, Tp, nq, nkv, scale, dtype16, stream};
    return launch_dq(r, "attn_bwd_scores", "attn_bwd_scores(resident)", att, lse, dQ, (long)ld_dq, stats, nullptr, nullptr, nullptr);
  }
  auto kfn = dtype16 == TCAVT_F16 ? attn_bwd_scores_kernel<true> : attn_bwd_scores_kernel<false>;
  hipLaunchKernelGGL(kfn, dim3((unsigned)((long)B * nq * (Tp / 64))), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(qkv_bf16), static_cast<const bf16_t*>(dO_bf16),
                     static_cast<bf16_t*>(dS_bf16), static_cast<bf16_t*>(PT_bf16), static_cast<bf16_t*>(dST_bf16), dQ, (long)ld_dq,
                     stats, kv_len, T, Tp, nq, nkv, scale, lse, static_cast<const bf16_t*>(att));
  TCAVT_CHECK_LAUNCH("attn_bwd_scores");
  return TCAVT_OK;
}

extern "C" int tcavt_attn_bwd_dkv(const void* qkv_bf16, const void* dO_bf16, const float* stats, float* g32,
                                  const int32_t* kv_len, int B, int T, int Tp, int nq, int nkv, int head_dim, float scale,
                                  int dtype16, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(qkv_bf16 && dO_bf16 && stats && g32 && kv_len && B > 0 && T > 0 && is16(dtype16), "attn_bwd_dkv: bad args");
  TCAVT_CHECK_ARG(head_dim == 64 && nkv > 0 && nq % nkv == 0, "attn_bwd_dkv: head_dim 64 and nq %% nkv == 0 required");
  TCAVT_CHECK_ARG(Tp >= T && Tp - T < 64 && Tp % 64 == 0, "attn_bwd_dkv: Tp must be T rounded up to a multiple of 64");
  TCAVT_CHECK_ARG(aligned16(qkv_bf16) && aligned16(dO_bf16) && aligned16(stats), "attn_bwd_dkv: 16-byte alignment required");
  if (Tp <= 256 && !resident_off()) {  // the query side of a whole head fits in LDS: no query-block loop
    const ResidentArgs r = {qkv_bf16, dO_bf16, kv_len, B, T, Tp, nq, nkv, scale, dtype16, stream};
    return launch_dkv_res(r, "attn_bwd_dkv", "attn_bwd_dkv(resident)", stats, g32, nullptr, nullptr, nullptr);
  }
  auto kfn = dtype16 == TCAVT_F16 ? attn_bwd_dkv_kernel<true> : attn_bwd_dkv_kernel<false>;
  hipLaunchKernelGGL(kfn, dim3((unsigned)((long)B * nkv * (Tp / 64))), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(qkv_bf16), static_cast<const bf16_t*>(dO_bf16),
                     stats, g32, kv_len, T, Tp, nq, nkv, scale);
  TCAVT_CHECK_LAUNCH("attn_bwd_dkv");
  return TCAVT_OK;
}

// Whole attention backward of the LoRA-trainable variant in its resident form: two launches, 16-bit output, no fp32 scratch
extern "C" int tcavt_attn_bwd_resident(const void* qkv16, const void* dO16, const void* att16, const float* lse, void* g_qkv16,
                                       float* stats, const float* rope_cos, const float* rope_sin, const int32_t* kv_len, int B,
                                       int T, int nq, int nkv, int head_dim, float scale, int dtype16, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(qkv16 && dO16 && att16 && lse && g_qkv16 && stats && rope_cos && rope_sin && kv_len && B > 0 && T > 0 && is16(dtype16),
                  "attn_bwd_resident: bad args");
  TCAVT_CHECK_ARG(head_dim == 64 && nkv > 0 && nq % nkv == 0, "attn_bwd_resident: head_dim 64 and nq %% nkv == 0 required");
  TCAVT_CHECK_ARG(tcavt_attn_bwd_resident_ok(T, nq, nkv), "attn_bwd_resident: T=%d, nq / nkv = %d outside the resident form (T <= 256, 16 %% (nq / nkv) == 0)", T, nq / nkv);
  TCAVT_CHECK_ARG(aligned16(qkv16) && aligned16(dO16) && aligned16(att16) && aligned16(stats) && aligned16(g_qkv16),
                  "attn_bwd_resident: 16-byte alignment required");
  const ResidentArgs r = {qkv16, dO16, kv_len, B, T, (T + 63) & ~63, nq, nkv, scale, dtype16, stream};
  TCAVT_TRY(launch_dq(r, "attn_bwd_resident", "attn_bwd_resident(dq)", att16, lse, nullptr, 0L, stats, g_qkv16, rope_cos, rope_sin));
  return launch_dkv_res(r, "attn_bwd_resident", "attn_bwd_resident(dkv)", stats, nullptr, g_qkv16, rope_cos, rope_sin);
}

extern "C" int tcavt_attn_bwd_resident_ok(int T, int nq, int nkv) { return T > 0 && T <= 256 && group_ok(nq, nkv); }

static std::string launch_name(const char* who, const char* part) { return std::string(who) + part; }

// The same backward in chunks of 256 keys / queries (attn_bwd_dq_long_kernel, attn_bwd_dkv_long_kernel).  Neither kernel
// depends on T: the LDS images are those of one chunk, both walk (T + 255) / 256 chunks, every row index is a long.
// `who` names the entry point in the messages, `max_T` is its cap (tcavt_attn_bwd_long: 544, tcavt_attn_bwd_stream: 2048).
static int attn_bwd_chunked(const char* who, int max_T, const void* qkv16, const void* dO16, const void* att16, const float* lse,
                            void* g_qkv16, float* stats, const float* rope_cos, const float* rope_sin, const int32_t* kv_len, int B,
                            int T, int nq, int nkv, int head_dim, float scale, int dtype16, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(qkv16 && dO16 && att16 && lse && g_qkv16 && stats && rope_cos && rope_sin && kv_len && B > 0 && T > 0 && is16(dtype16),
                  "%s: bad args", who);
  TCAVT_CHECK_ARG(head_dim == 64 && nkv > 0 && nq > 0 && nq % nkv == 0, "%s: head_dim 64 and nq %% nkv == 0 required", who);
  TCAVT_CHECK_ARG(T <= max_T && group_ok(nq, nkv),
                  "%s: T=%d, nq / nkv = %d outside the chunked form (T <= %d, 16 %% (nq / nkv) == 0)", who, T, nq / nkv, max_T);
  TCAVT_CHECK_ARG(aligned16(qkv16) && aligned16(dO16) && aligned16(att16) && aligned16(stats) && aligned16(g_qkv16),
                  "%s: 16-byte alignment required", who);
  const bool f16 = dtype16 == TCAVT_F16;
  const int group = nq / nkv, U = group < 2 ? group : 2;
  typedef void (*dq_fn)(const bf16_t*, const bf16_t*, const bf16_t*, const float*, float*, const int*, int, int, int, int, int, float,
                        bf16_t*, const float*, const float*);
  static const dq_fn kqs[2][2] = {{attn_bwd_dq_long_kernel<false, 1>, attn_bwd_dq_long_kernel<false, 2>},
                                  {attn_bwd_dq_long_kernel<true, 1>, attn_bwd_dq_long_kernel<true, 2>}};
  const dq_fn kq = kqs[f16][U - 1];
  auto kr = f16 ? attn_bwd_dkv_long_kernel<true> : attn_bwd_dkv_long_kernel<false>;
  constexpr int lds_q = attn_bwd_dq_lds(ABL_CHUNK), lds_kv = attn_bwd_dkv_res_lds(ABL_CHUNK);  // one chunk's images
  static bool q_limit_set[2][2] = {{false, false}, {false, false}}, kv_limit_set[2] = {false, false};
  TCAVT_TRY(dyn_lds_limit(reinterpret_cast<const void*>(kq), lds_q, who, q_limit_set[f16][U - 1]));
  TCAVT_TRY(dyn_lds_limit(reinterpret_cast<const void*>(kr), lds_kv, who, kv_limit_set[f16]));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bf16_t* q_ = static_cast<const bf16_t*>(qkv16);
  const bf16_t* g_ = static_cast<const bf16_t*>(dO16);
  const int QC = ABL_CHUNK * U / group;
  const int nqc = (T + QC - 1) / QC, nkc = (T + ABL_CHUNK - 1) / ABL_CHUNK, nbj = B * nkv;
  hipLaunchKernelGGL(kq, dim3((unsigned)(nbj * nqc)), dim3(ABQ_WAVES * 64), lds_q, st, q_, g_, static_cast<const bf16_t*>(att16), lse,
                     stats, kv_len, T, nq, nkv, nqc, nbj, scale, static_cast<bf16_t*>(g_qkv16), rope_cos, rope_sin);
  TCAVT_CHECK_LAUNCH(launch_name(who, "(dq)").c_str());
  hipLaunchKernelGGL(kr, dim3((unsigned)(nbj * nkc)), dim3(1024), lds_kv, st, q_, g_, static_cast<const float*>(stats), kv_len, T, nq,
                     nkv, nbj, scale, static_cast<bf16_t*>(g_qkv16), rope_cos, rope_sin);
  TCAVT_CHECK_LAUNCH(launch_name(who, "(dkv)").c_str());
  return TCAVT_OK;
}

extern "C" int tcavt_attn_bwd_long(const void* qkv16, const void* dO16, const void* att16, const float* lse, void* g_qkv16,
                                   float* stats, const float* rope_cos, const float* rope_sin, const int32_t* kv_len, int B, int T,
                                   int nq, int nkv, int head_dim, float scale, int dtype16, tcavt_stream_t stream) {
  return attn_bwd_chunked("attn_bwd_long", ABL_MAX_T, qkv16, dO16, att16, lse, g_qkv16, stats, rope_cos, rope_sin, kv_len, B, T, nq,
                          nkv, head_dim, scale, dtype16, stream);
}

// where the dispatch (llm_backward.attn_bwd_composed, tcavt_llama_stack_backward) takes the chunked form
extern "C" int tcavt_attn_bwd_long_ok(int T, int nq, int nkv) { return T > 256 && T <= ABL_MAX_T && group_ok(nq, nkv); }

// The chunked form beyond 544 (stage 1 truncates its text to 1024 tokens: L up to 1040): the same two launches under the
// cap of the streaming forward, TCAVT_ATTN_STREAM_MAX_L
extern "C" int tcavt_attn_bwd_stream(const void* qkv16, const void* dO16, const void* att16, const float* lse, void* g_qkv16,
                                     float* stats, const float* rope_cos, const float* rope_sin, const int32_t* kv_len, int B, int T,
                                     int nq, int nkv, int head_dim, float scale, int dtype16, tcavt_stream_t stream) {
  return attn_bwd_chunked("attn_bwd_stream", TCAVT_ATTN_STREAM_MAX_L, qkv16, dO16, att16, lse, g_qkv16, stats, rope_cos, rope_sin,
                          kv_len, B, T, nq, nkv, head_dim, scale, dtype16, stream);
}

extern "C" int tcavt_attn_bwd_stream_ok(int T, int nq, int nkv) {
  return T > ABL_MAX_T && T <= TCAVT_ATTN_STREAM_MAX_L && group_ok(nq, nkv);
}

