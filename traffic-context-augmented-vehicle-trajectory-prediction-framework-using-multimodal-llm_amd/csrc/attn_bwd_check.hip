// Cross-checks of the attention backward (csrc/attn_bwd.hip), not product paths: the scalar-FMA kernel, and the row-wise
// middle and the pack kernel of the GEMM-composed forms (llm_backward.attn_bwd_composed, scores = "gemm" / "gemm_tiles").
#include "common.hpp"

namespace tcavt {

// ---------------------------------------------------------------------------
// (cross-check kernel) Causal GQA attention backward, head_dim 64.  One workgroup per (sample, query head, block of QB = 32 query rows).
//   P = softmax(scale * q K^T) over keys c < min(i + 1, kv_len[b]);   dP = dO V^T;   dS = scale * P * (dP - rowsum(P dP))
//   dQ_i = sum_c dS_ic K_c  (written);   dK_c += sum_i dS_ic q_i,  dV_c += sum_i P_ic dO_i  (float atomics: the four
//   query heads of a group and the query blocks all add into the same key rows).
// q, k, v are read from the forward's rotated q|k|v buffer [B*T, (nq + 2 nkv) * 64] (bf16), dO from [B*T, nq*64] (bf16);
// g32 is the fp32 gradient in the q|k|v layout, zeroed by the caller.
// ---------------------------------------------------------------------------
constexpr int AB_QB = 32, AB_HD = 64, AB_LDK = 66;  // K/V rows padded to 33 dwords (conflict-free down a column)

__global__ __launch_bounds__(256) void attn_causal_gqa_bwd_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dO,
                                                                  float* __restrict__ g32, const int* __restrict__ kv_len,
                                                                  int T, int nq, int nkv, float scale, int nqb) {
  extern __shared__ float sm[];
  const int blk = blockIdx.x;
  const int qb = blk % nqb, h = (blk / nqb) % nq, b = blk / (nqb * nq);
  const int j = h / (nq / nkv);
  const int q0 = qb * AB_QB;
  const int klen = min(kv_len[b], T);
  const int nk = min(min(q0 + AB_QB, T), klen);  // keys any row of this block can see
  const int nqkv = (nq + 2 * nkv) * AB_HD;
  float* S = sm;                                   // [QB][nk]  scores -> P
  float* D = S + AB_QB * nk;                       // [QB][nk]  dP -> dS
  float* qs = D + AB_QB * nk;                      // [QB][65]
  float* gs = qs + AB_QB * (AB_HD + 1);            // [QB][65]
  bf16_t* ks = reinterpret_cast<bf16_t*>(gs + AB_QB * (AB_HD + 1));  // [nk][66]
  bf16_t* vs = ks + (long)nk * AB_LDK;                                // [nk][66]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long row0 = (long)b * T;
  for (int id = tid; id < AB_QB * AB_HD; id += 256) {
    const int i = id >> 6, e = id & 63;
    const bool ok = q0 + i < T;
    qs[i * 65 + e] = ok ? bf16_to_f32(qkv[(row0 + q0 + i) * nqkv + h * AB_HD + e]) : 0.f;
    gs[i * 65 + e] = ok ? bf16_to_f32(dO[(row0 + q0 + i) * (long)(nq * AB_HD) + h * AB_HD + e]) : 0.f;
  }
  for (int id = tid; id < nk * AB_HD; id += 256) {
    const int c = id >> 6, e = id & 63;
    ks[c * AB_LDK + e] = qkv[(row0 + c) * nqkv + (nq + j) * AB_HD + e];
    vs[c * AB_LDK + e] = qkv[(row0 + c) * nqkv + (nq + nkv + j) * AB_HD + e];
  }
  __syncthreads();
  for (int ij = tid; ij < AB_QB * nk; ij += 256) {
    const int i = ij / nk, c = ij - i * nk;
    float s = -1e30f, d = 0.f;
    if (q0 + i < T && c < min(q0 + i + 1, klen)) {
      s = 0.f;
      const float* qr = qs + i * 65;
      const float* gr = gs + i * 65;
      const unsigned int* kr = reinterpret_cast<const unsigned int*>(ks + c * AB_LDK);
      const unsigned int* vr = reinterpret_cast<const unsigned int*>(vs + c * AB_LDK);
#pragma unroll 8
      for (int e2 = 0; e2 < AB_HD / 2; ++e2) {
        const unsigned int kk = kr[e2], vv = vr[e2];
        s = fmaf(qr[2 * e2], __uint_as_float(kk << 16), s);
        s = fmaf(qr[2 * e2 + 1], __uint_as_float(kk & 0xffff0000u), s);
        d = fmaf(gr[2 * e2], __uint_as_float(vv << 16), d);
        d = fmaf(gr[2 * e2 + 1], __uint_as_float(vv & 0xffff0000u), d);
      }
      s *= scale;
    }
    S[ij] = s;
    D[ij] = d;
  }
  __syncthreads();
  for (int i = wave; i < AB_QB; i += 4) {
    float* row = S + i * nk;
    float* drow = D + i * nk;
    float m = -1e30f;
    for (int c = lane; c < nk; c += 64) m = fmaxf(m, row[c]);
    m = wave_max(m);
    float sum = 0.f;
    for (int c = lane; c < nk; c += 64) {
      const float e = row[c] > -1e29f ? __expf(row[c] - m) : 0.f;
      row[c] = e;
      sum += e;
    }
    sum = wave_sum(sum);
    const float inv = sum > 0.f ? 1.f / sum : 0.f;
    float dot = 0.f;
    for (int c = lane; c < nk; c += 64) {
      row[c] *= inv;
      dot = fmaf(row[c], drow[c], dot);
    }
    dot = wave_sum(dot);
    for (int c = lane; c < nk; c += 64) drow[c] = row[c] * (drow[c] - dot) * scale;
  }
  __syncthreads();
  for (int id = tid; id < AB_QB * AB_HD; id += 256) {  // dQ
    const int i = id >> 6, e = id & 63;
    if (q0 + i >= T) continue;
    const float* dr = D + i * nk;
    float a = 0.f;
#pragma unroll 8
    for (int c = 0; c < nk; ++c) a = fmaf(dr[c], bf16_to_f32(ks[c * AB_LDK + e]), a);
    g32[(row0 + q0 + i) * nqkv + h * AB_HD + e] = a;
  }
  for (int id = tid; id < nk * AB_HD; id += 256) {  // dK, dV
    const int c = id >> 6, e = id & 63;
    float a = 0.f, v = 0.f;
#pragma unroll 8
    for (int i = 0; i < AB_QB; ++i) {
      a = fmaf(D[i * nk + c], qs[i * 65 + e], a);
      v = fmaf(S[i * nk + c], gs[i * 65 + e], v);
    }
    atomicAdd(g32 + (row0 + c) * nqkv + (nq + j) * AB_HD + e, a);
    atomicAdd(g32 + (row0 + c) * nqkv + (nq + nkv + j) * AB_HD + e, v);
  }
}


// ---------------------------------------------------------------------------
// Composed attention backward (the production path; the scalar kernel above is its cross-check): the five products run
// on the batched MFMA GEMM, and this kernel is the row-wise middle.  Row r = (b * nq + h) * T + i of S (already scaled
// scores, fp32 [.., Tp]) and dP = dO V^T (fp32):
//   P = softmax(S[:nv]), nv = min(i + 1, kv_len[b]);   dS = scale * P * (dP - sum P dP)
// both written as bf16 rows of Tp columns, zero beyond nv (the GEMMs that consume them contract over all Tp columns).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void causal_softmax_bwd_rows_kernel(const float* __restrict__ S, const float* __restrict__ dP,
                                                                      bf16_t* __restrict__ P, bf16_t* __restrict__ dS,
                                                                      const int* __restrict__ kv_len, int T, int Tp, int nq,
                                                                      float scale, long rows) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int i = (int)(row % T);
  const int b = (int)(row / ((long)T * nq));
  const int nv = min(i + 1, min(kv_len[b], T));
  const f32x4* s4 = reinterpret_cast<const f32x4*>(S + row * Tp);
  const f32x4* d4 = reinterpret_cast<const f32x4*>(dP + row * Tp);
  const int nv4 = (nv + 3) >> 2, n4 = Tp >> 2;
  float m = -1e30f;
  for (int q = lane; q < nv4; q += 64) {
    const f32x4 v = s4[q];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * q + e < nv) m = fmaxf(m, v[e]);
  }
  m = wave_max(m);
  float sum = 0.f, dot = 0.f;
  for (int q = lane; q < nv4; q += 64) {
    const f32x4 v = s4[q], dd = d4[q];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * q + e < nv) {
        const float ex = __expf(v[e] - m);
        sum += ex;
        dot = fmaf(ex, dd[e], dot);
      }
  }
  sum = wave_sum(sum);
  dot = wave_sum(dot);
  const float inv = sum > 0.f ? 1.f / sum : 0.f;
  dot *= inv;
  u32x2* po = reinterpret_cast<u32x2*>(P + row * Tp);
  u32x2* so = reinterpret_cast<u32x2*>(dS + row * Tp);
  for (int q = lane; q < n4; q += 64) {
    float pv[4] = {0.f, 0.f, 0.f, 0.f}, dv[4] = {0.f, 0.f, 0.f, 0.f};
    if (q < nv4) {
      const f32x4 v = s4[q], dd = d4[q];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * q + e < nv) {
          pv[e] = __expf(v[e] - m) * inv;
          dv[e] = scale * pv[e] * (dd[e] - dot);
        }
    }
    const u32x2 pb = {pack_bf16x2(pv[0], pv[1]), pack_bf16x2(pv[2], pv[3])};
    const u32x2 db = {pack_bf16x2(dv[0], dv[1]), pack_bf16x2(dv[2], dv[3])};
    po[q] = pb;
    so[q] = db;
  }
}


// The same row arithmetic, tiled: one workgroup per (sample, query head, block of 64 queries) writes dS (row-major, for
// dQ = dS K) and the TRANSPOSED tiles P^T, dS^T (for dV = P^T dO, dK = dS^T q) through LDS, so that no separate
// transposition pass (and no row-major P) is needed.  Key blocks above the causal diagonal are never touched: the
// three outputs must be zero-initialised once by the caller and stay zero there whatever kv_len is.
__global__ __launch_bounds__(256) void causal_softmax_bwd_tiles_kernel(const float* __restrict__ S, const float* __restrict__ dP,
                                                                       bf16_t* __restrict__ dS, bf16_t* __restrict__ PT,
                                                                       bf16_t* __restrict__ dST, const int* __restrict__ kv_len,
                                                                       int T, int Tp, int nq, float scale) {
  __shared__ float st_m[64], st_inv[64], st_dot[64];
  __shared__ int st_nv[64];
  __shared__ bf16_t tP[64][66], tD[64][66];
  const int nqb = Tp >> 6;
  const int qb = blockIdx.x % nqb;
  const long bh = blockIdx.x / nqb;
  const int b = (int)(bh / nq);
  const int klen = min(kv_len[b], T);
  const int q0 = qb * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int rr = 0; rr < 16; ++rr) {  // row statistics: a wave per row
    const int r = wave * 16 + rr, i = q0 + r;
    const int nv = i < T ? min(i + 1, klen) : 0;
    const f32x4* s4 = reinterpret_cast<const f32x4*>(S + (bh * T + i) * Tp);
    const f32x4* d4 = reinterpret_cast<const f32x4*>(dP + (bh * T + i) * Tp);
    const int nv4 = (nv + 3) >> 2;
    float m = -1e30f;
    for (int q = lane; q < nv4; q += 64) {
      const f32x4 v = s4[q];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * q + e < nv) m = fmaxf(m, v[e]);
    }
    m = wave_max(m);
    float sum = 0.f, dot = 0.f;
    for (int q = lane; q < nv4; q += 64) {
      const f32x4 v = s4[q], dd = d4[q];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * q + e < nv) {
          const float ex = __expf(v[e] - m);
          sum += ex;
          dot = fmaf(ex, dd[e], dot);
        }
    }
    sum = wave_sum(sum);
    dot = wave_sum(dot);
    if (lane == 0) {
      const float inv = sum > 0.f ? 1.f / sum : 0.f;
      st_m[r] = m;
      st_inv[r] = inv;
      st_dot[r] = dot * inv;
      st_nv[r] = nv;
    }
  }
  __syncthreads();
  for (int kb = 0; kb <= qb; ++kb) {
    const int c = kb * 64 + lane;
    for (int rr = 0; rr < 16; ++rr) {
      const int r = wave * 16 + rr, i = q0 + r;
      float pv = 0.f, dv = 0.f;
      if (c < st_nv[r]) {
        const long o = (bh * T + i) * Tp + c;
        pv = __expf(S[o] - st_m[r]) * st_inv[r];
        dv = scale * pv * (dP[o] - st_dot[r]);
      }
      const bf16_t db = f32_to_bf16(dv);
      if (i < T) dS[(bh * T + i) * Tp + c] = db;
      tP[r][lane] = f32_to_bf16(pv);
      tD[r][lane] = db;
    }
    __syncthreads();
    for (int cc = wave * 16; cc < wave * 16 + 16; ++cc) {  // transposed tiles: key row kb*64 + cc, 64 queries across the lanes
      const long o = (bh * Tp + kb * 64 + cc) * Tp + q0 + lane;
      PT[o] = tP[lane][cc];
      dST[o] = tD[lane][cc];
    }
    __syncthreads();
  }
}


// G3 fp32 [M, 3 * nq * 64] = dQ | dK per QUERY head | dV per QUERY head  ->  bf16 [M, (nq + 2 nkv) * 64]: the query heads of
// a group are summed into their key / value head, q and k get the transposed RoPE rotation (rope_bwd_pack_kernel).
__global__ __launch_bounds__(256) void gqa_rope_bwd_pack_kernel(const float* __restrict__ G3, bf16_t* __restrict__ out,
                                                                const float* __restrict__ cosT, const float* __restrict__ sinT,
                                                                long M, int nq, int nkv, int L) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int heads = nq + 2 * nkv;
  if (idx >= M * heads * 32) return;
  const int w = (int)(idx & 31);
  const int oh = (int)((idx >> 5) % heads);
  const long row = idx / ((long)heads * 32);
  const int grp = nq / nkv;
  const float* g = G3 + row * (3L * nq * 64);
  float a = 0.f, b = 0.f;
  bool rot = true;
  if (oh < nq) {
    a = g[oh * 64 + w];
    b = g[oh * 64 + w + 32];
  } else {
    const bool isv = oh >= nq + nkv;
    const int j = oh - nq - (isv ? nkv : 0);
    const float* src = g + (isv ? 2 : 1) * nq * 64 + j * grp * 64;
    for (int q = 0; q < grp; ++q) {
      a += src[q * 64 + w];
      b += src[q * 64 + w + 32];
    }
    rot = !isv;
  }
  float o1 = a, o2 = b;
  if (rot) {
    const int pos = (int)(row % L);
    const float cs = cosT[pos * 32 + w], sn = sinT[pos * 32 + w];
    o1 = a * cs + b * sn;
    o2 = b * cs - a * sn;
  }
  out[row * (heads * 64L) + oh * 64 + w] = f32_to_bf16(o1);
  out[row * (heads * 64L) + oh * 64 + w + 32] = f32_to_bf16(o2);
}

static size_t attn_bwd_lds(int T) {
  return (size_t)2 * AB_QB * T * 4 + (size_t)2 * AB_QB * (AB_HD + 1) * 4 + (size_t)2 * T * AB_LDK * 2;
}

}  // namespace tcavt

using namespace tcavt;

extern "C" int tcavt_attn_causal_gqa_bwd(const void* qkv_bf16, const void* dO_bf16, float* g32, const int32_t* kv_len, int B,
                                         int T, int nq, int nkv, int head_dim, float scale, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(qkv_bf16 && dO_bf16 && g32 && kv_len && B > 0 && T > 0, "attn_causal_gqa_bwd: bad args");
  TCAVT_CHECK_ARG(head_dim == 64 && nkv > 0 && nq % nkv == 0, "attn_causal_gqa_bwd: head_dim 64 and nq %% nkv == 0 required");
  const size_t lds = attn_bwd_lds(T);
  TCAVT_CHECK_ARG(lds <= 160 * 1024, "attn_causal_gqa_bwd: T=%d needs %zu bytes of LDS (limit 160 KB, T <= 280)", T, lds);
  static bool limit_set = false;
  const int rc = dyn_lds_limit(reinterpret_cast<const void*>(attn_causal_gqa_bwd_kernel), 160 * 1024, "attn_causal_gqa_bwd", limit_set);
  if (rc != TCAVT_OK) return rc;
  const int nqb = (T + AB_QB - 1) / AB_QB;
  hipLaunchKernelGGL(attn_causal_gqa_bwd_kernel, dim3((unsigned)(B * nq * nqb)), dim3(256), lds, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(qkv_bf16), static_cast<const bf16_t*>(dO_bf16), g32, kv_len, T, nq, nkv, scale,
                     nqb);
  TCAVT_CHECK_LAUNCH("attn_causal_gqa_bwd");
  return TCAVT_OK;
}

extern "C" int tcavt_causal_softmax_bwd_rows(const float* S, const float* dP, void* P_bf16, void* dS_bf16,
                                             const int32_t* kv_len, int B, int T, int Tp, int nq, float scale,
                                             tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(S && dP && P_bf16 && dS_bf16 && kv_len && B > 0 && T > 0 && Tp >= T && Tp % 4 == 0 && nq > 0, "causal_softmax_bwd_rows: bad args");
  TCAVT_CHECK_ARG(aligned16(S) && aligned16(dP) && aligned16(P_bf16) && aligned16(dS_bf16), "causal_softmax_bwd_rows: 16-byte alignment required");
  const long rows = (long)B * nq * T;
  hipLaunchKernelGGL(causal_softmax_bwd_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), S, dP, static_cast<bf16_t*>(P_bf16), static_cast<bf16_t*>(dS_bf16),
                     kv_len, T, Tp, nq, scale, rows);
  TCAVT_CHECK_LAUNCH("causal_softmax_bwd_rows");
  return TCAVT_OK;
}

extern "C" int tcavt_gqa_rope_bwd_pack(const float* G3, void* out_bf16, const float* rope_cos, const float* rope_sin, int64_t M,
                                       int nq, int nkv, int head_dim, int L, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(G3 && out_bf16 && rope_cos && rope_sin && M > 0 && L > 0, "gqa_rope_bwd_pack: bad args");
  TCAVT_CHECK_ARG(head_dim == 64 && nkv > 0 && nq % nkv == 0, "gqa_rope_bwd_pack: head_dim 64 and nq %% nkv == 0 required");
  const long n = (long)M * (nq + 2 * nkv) * 32;
  hipLaunchKernelGGL(gqa_rope_bwd_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     G3, static_cast<bf16_t*>(out_bf16), rope_cos, rope_sin, (long)M, nq, nkv, L);
  TCAVT_CHECK_LAUNCH("gqa_rope_bwd_pack");
  return TCAVT_OK;
}

extern "C" int tcavt_causal_softmax_bwd_tiles(const float* S, const float* dP, void* dS_bf16, void* PT_bf16, void* dST_bf16,
                                              const int32_t* kv_len, int B, int T, int Tp, int nq, float scale,
                                              tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(S && dP && dS_bf16 && PT_bf16 && dST_bf16 && kv_len && B > 0 && T > 0 && nq > 0, "causal_softmax_bwd_tiles: bad args");
  TCAVT_CHECK_ARG(Tp >= T && Tp - T < 64 && Tp % 64 == 0, "causal_softmax_bwd_tiles: Tp must be T rounded up to a multiple of 64");
  TCAVT_CHECK_ARG(aligned16(S) && aligned16(dP), "causal_softmax_bwd_tiles: 16-byte alignment required");
  hipLaunchKernelGGL(causal_softmax_bwd_tiles_kernel, dim3((unsigned)((long)B * nq * (Tp / 64))), dim3(256), 0,
                     static_cast<hipStream_t>(stream), S, dP, static_cast<bf16_t*>(dS_bf16), static_cast<bf16_t*>(PT_bf16),
                     static_cast<bf16_t*>(dST_bf16), kv_len, T, Tp, nq, scale);
  TCAVT_CHECK_LAUNCH("causal_softmax_bwd_tiles");
  return TCAVT_OK;
}

