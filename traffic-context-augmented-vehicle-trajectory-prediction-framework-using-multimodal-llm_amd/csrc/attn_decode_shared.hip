// Decode attention for n continuations that share their prompt's cache (include/tcavt.h: tcavt_attn_decode_shared).
//
// generate_batch(num_return_sequences = n) prefills a prompt once; with share_prefix the prompt's K / V rows stay where the
// prefill wrote them ([B][prefix_lmax][nkv * 64], read only) and each of the R = B * n decode rows owns a suffix cache of its
// generated tokens only.  A query attends to [ shared prefix | own suffix | its new token ].
//
// attn_decode_kernel (csrc/attn_decode.hip) reads every cached row once per (row, query head).  Here a prefix row is fetched once
// per (prompt, kv head, block of 32 queries): the n * group queries that share a prompt's kv head -- query (j, g) =
// continuation j, head g of the group, number j * group + g -- take the place of the sequence positions of
// attn_causal_gqa_stream_kernel (csrc/attention.hip), and per 32-key tile the arithmetic is that kernel's:
//     S^T = K . Q^T     v_mfma_f32_32x32x16, the key on the accumulator row, the query on the lane
//     O^T += V^T . P^T  the S^T accumulator, converted in place to fp16, is the B operand
// with an online softmax in fp32 (exp2, log2 e folded into the scale).  There is no causal mask, only key < prefix_len[b].
//
// One workgroup of DS_W waves per (prompt, kv head, query block).  Wave w takes the key tiles w, w + DS_W, ...: its K fragments
// come straight from global memory (a key row is read by one wave only), its V tile is transposed through a wave-private LDS
// buffer.  The waves' (m, l, O^T) meet in LDS in a fixed order (a halving tree), so a launch repeats bit for bit.  Rows at or
// beyond prefix_len[b] are never loaded: their loads are clamped to the last valid row and their V is staged as zeros.
//
// The suffix (at most suffix_lmax - 1 keys of the row, and the new token taken from qkv) keeps the VALU form of
// attn_decode_kernel, one wave per (continuation, heads of the group): a key row is loaded once for the group's heads, a round of
// 64 keys keeps its scores in registers and the rounds run an online softmax of their own.  Then the prefix partial and the
// suffix partial are merged by log-sum-exp in fp32 -- M = max(m_prefix, m_suffix), O = (O_prefix * exp2(m_prefix - M) + O_suffix *
// exp2(m_suffix - M)) / l; the probabilities are carried as fp16 on both sides.  The wave that has the group's first head
// appends the qkv row's k | v bits to suffix row t.
#include "common.hpp"

namespace tcavt {

constexpr int DS_W = 8;                    // waves per workgroup (a power of two)
constexpr int DS_VS = 32 + 4;              // V^T row stride (elements): 8-byte reads of 32 rows without bank conflicts
constexpr int DS_STAGE = 64 * DS_VS * 2;   // bytes of a wave's V^T tile
constexpr int DS_OS = 64 + 1;              // row stride of the merged prefix output (floats)
constexpr int DS_H = 4;                    // heads of a group a wave serves at once in the suffix pass
constexpr int DS_SUFFIX_MAX = TCAVT_ATTN_DECODE_SHARED_MAX_SUFFIX;  // the longest suffix the entry accepts
static_assert((DS_W / 2) * 32 * 64 * 4 <= DS_W * DS_STAGE, "the halving tree's slots lie in the staging area");

template <bool F16>
__global__ __launch_bounds__(DS_W * 64) void attn_decode_shared_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ pk,
                                                                       const bf16_t* __restrict__ pv, const int* __restrict__ plen_p,
                                                                       bf16_t* __restrict__ sk, bf16_t* __restrict__ sv,
                                                                       const int* __restrict__ pos, bf16_t* __restrict__ out, int n,
                                                                       int nq, int nkv, int plmax, int slmax, int nblk,
                                                                       float scale_log2e, int out_frag) {
  __shared__ __attribute__((aligned(16))) char stage[DS_W * DS_STAGE];
  __shared__ float mstat[DS_W][32], lstat[DS_W][32];  // per wave and query: running maximum (log2 domain) and sum
  __shared__ float opre[32 * DS_OS];                  // merged prefix O (unnormalised), [query][feature]
  __shared__ float gstat[2][32];                      // its maximum and sum
  const int group = nq / nkv;
  const int blk = blockIdx.x % nblk, bj = blockIdx.x / nblk;
  const int b = bj / nkv, kvh = bj % nkv;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int ld = (nq + 2 * nkv) * 64, w = nkv * 64;
  const int nQ = n * group;  // queries of this (prompt, kv head)
  const int plen_raw = plen_p[b];
  const int plen = min(max(plen_raw, 0), plmax);
  const int tiles = (plen + 31) >> 5;

  // ---- prefix: this lane's query (a padded lane loads the last real query and stores nothing)
  bf16x8 qf[4];
  {
    const int qx = min(blk * 32 + r, nQ - 1);
    const bf16_t* qrow = qkv + (long)(b * n + qx / group) * ld + (kvh * group + qx % group) * 64;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(qrow + s * 16 + hh * 8);
  }
  f32x16 o0, o1;
#pragma unroll
  for (int i = 0; i < 16; ++i) { o0[i] = 0.f; o1[i] = 0.f; }
  float mrun = -1e30f, lrun = 0.f;
  const bf16_t* kb = pk + (long)b * plmax * w + kvh * 64;
  const bf16_t* vb = pv + (long)b * plmax * w + kvh * 64;
  bf16_t* Vt = reinterpret_cast<bf16_t*>(stage + wave * DS_STAGE);
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  const int iters = (tiles + DS_W - 1) / DS_W;  // (uniform over the workgroup: the barriers below)
  for (int it = 0; it < iters; ++it) {
    const int kt = it * DS_W + wave;
    const bool has = kt < tiles;  // (uniform over the wave)
    bf16x8 kf[4];
    u32x4 va[2], vc[2];
    if (has) {
      const int key = min(kt * 32 + r, plen - 1);
#pragma unroll
      for (int s = 0; s < 4; ++s) kf[s] = *reinterpret_cast<const bf16x8*>(kb + (long)key * w + s * 16 + hh * 8);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int idx = lane + i * 64;
        const int r0 = kt * 32 + 2 * (idx >> 3), c = idx & 7;
        va[i] = *reinterpret_cast<const u32x4*>(vb + (long)min(r0, plen - 1) * w + c * 8);
        vc[i] = *reinterpret_cast<const u32x4*>(vb + (long)min(r0 + 1, plen - 1) * w + c * 8);
      }
    }
    if (it > 0) __syncthreads();  // the wave's lanes are done with the previous tile
    if (has) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int idx = lane + i * 64;
        const int r0 = 2 * (idx >> 3), c = idx & 7;
        const u32x4 a = (kt * 32 + r0 < plen) ? va[i] : zero4, bb = (kt * 32 + r0 + 1 < plen) ? vc[i] : zero4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          unsigned int lo, hi;
          if constexpr (F16) {
            lo = (a[e] & 0xffffu) | (bb[e] << 16);
            hi = (a[e] >> 16) | (bb[e] & 0xffff0000u);
          } else {
            lo = bf16pair_to_f16pair(a[e] & 0xffffu, bb[e] & 0xffffu);
            hi = bf16pair_to_f16pair(a[e] >> 16, bb[e] >> 16);
          }
          *reinterpret_cast<unsigned int*>(Vt + (c * 8 + 2 * e) * DS_VS + r0) = lo;
          *reinterpret_cast<unsigned int*>(Vt + (c * 8 + 2 * e + 1) * DS_VS + r0) = hi;
        }
      }
    }
    __syncthreads();
    if (has) {
      f32x16 sacc;
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[i] = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if constexpr (F16)
          sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, kf[s]), __builtin_bit_cast(f16x8, qf[s]), sacc, 0, 0, 0);
        else
          sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[s], qf[s], sacc, 0, 0, 0);
      }
      // scale + tile max; per-element masks only on the tile that straddles prefix_len
      float p[16];
      if (kt * 32 + 32 <= plen) {
        float rmax = fmaxf(fmaxf(sacc[0], sacc[1]), sacc[2]);
#pragma unroll
        for (int i = 3; i + 1 < 16; i += 2) rmax = fmaxf(fmaxf(rmax, sacc[i]), sacc[i + 1]);
        rmax = fmaxf(rmax, sacc[15]);
        { float a, b2; halves(rmax, a, b2); rmax = fmaxf(a, b2); }
        const float mnew = fmaxf(mrun, rmax * scale_log2e);
        const float alpha = __builtin_amdgcn_exp2f(mrun - mnew);
        float psum = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          p[i] = __builtin_amdgcn_exp2f(fmaf(sacc[i], scale_log2e, -mnew));
          psum += p[i];
        }
        { float a, b2; halves(psum, a, b2); psum = a + b2; }
        lrun = lrun * alpha + psum;
        mrun = mnew;
#pragma unroll
        for (int i = 0; i < 16; ++i) { o0[i] *= alpha; o1[i] *= alpha; }
      } else {
        float tmax = -1e30f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int kk = kt * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
          p[i] = kk < plen ? sacc[i] * scale_log2e : -1e30f;
          tmax = fmaxf(tmax, p[i]);
        }
        { float a, b2; halves(tmax, a, b2); tmax = fmaxf(a, b2); }
        const float mnew = fmaxf(mrun, tmax);
        const float alpha = __builtin_amdgcn_exp2f(mrun - mnew);
        float psum = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          p[i] = (p[i] > -1e29f) ? __builtin_amdgcn_exp2f(p[i] - mnew) : 0.f;
          psum += p[i];
        }
        { float a, b2; halves(psum, a, b2); psum = a + b2; }
        lrun = lrun * alpha + psum;
        mrun = mnew;
#pragma unroll
        for (int i = 0; i < 16; ++i) { o0[i] *= alpha; o1[i] *= alpha; }
      }
      // O^T += V^T . P^T  (two 16-key k-steps; P registers 8 * s2 .. are the B operand)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const f16x8 pf = cvt8_f16(&p[8 * s2]);
        const int kbase = 16 * s2 + 4 * hh;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const bf16_t* vrow = Vt + (dt * 32 + r) * DS_VS + kbase;
          const u32x2 lo = *reinterpret_cast<const u32x2*>(vrow);
          const u32x2 hi = *reinterpret_cast<const u32x2*>(vrow + 8);
          const u32x4 vv = {lo[0], lo[1], hi[0], hi[1]};
          const f16x8 vf = __builtin_bit_cast(f16x8, vv);
          if (dt == 0) o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, o0, 0, 0, 0);
          else o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, o1, 0, 0, 0);
        }
      }
    }
  }

  // ---- the waves' partials meet: one maximum and one sum per query, then O^T over a halving tree in the staging area
  if (hh == 0) { mstat[wave][r] = mrun; lstat[wave][r] = lrun; }
  __syncthreads();  // (also: every wave is done with its V^T tile)
  float gm = -1e30f, gl = 0.f;
#pragma unroll
  for (int k = 0; k < DS_W; ++k) gm = fmaxf(gm, mstat[k][r]);
#pragma unroll
  for (int k = 0; k < DS_W; ++k) gl += lstat[k][r] * __builtin_amdgcn_exp2f(mstat[k][r] - gm);
  {
    const float f = __builtin_amdgcn_exp2f(mrun - gm);  // (a wave without a key tile: O = 0 whatever f is)
#pragma unroll
    for (int i = 0; i < 16; ++i) { o0[i] *= f; o1[i] *= f; }
  }
  float* red = reinterpret_cast<float*>(stage);
  for (int half = DS_W / 2; half >= 1; half >>= 1) {
    if (wave >= half && wave < 2 * half) {
      float* slot = red + (wave - half) * 2048;
#pragma unroll
      for (int i = 0; i < 16; ++i) { slot[i * 64 + lane] = o0[i]; slot[(16 + i) * 64 + lane] = o1[i]; }
    }
    __syncthreads();
    if (wave < half) {
      const float* slot = red + wave * 2048;
#pragma unroll
      for (int i = 0; i < 16; ++i) { o0[i] += slot[i * 64 + lane]; o1[i] += slot[(16 + i) * 64 + lane]; }
    }
    __syncthreads();
  }
  if (wave == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int d = (i & 3) + 8 * (i >> 2) + 4 * hh;
      opre[r * DS_OS + d] = o0[i];
      opre[r * DS_OS + 32 + d] = o1[i];
    }
    if (hh == 0) { gstat[0][r] = gm; gstat[1][r] = gl; }
  }
  __syncthreads();

  // ---- suffix + merge: one wave per (continuation, up to DS_H heads of the group that lie in this block): a key / value row is
  // loaded once for those heads.  attn_decode_kernel's lane = (key g8 of an 8-key row group, 16-byte column c); a round of 64 keys
  // keeps its scores in registers (after the three shuffles every lane of a key's 8 holds the key's score), so there is no score
  // buffer: an online softmax over the rounds, K and V of a round requested together.
  const int g8 = lane >> 3, c = lane & 7;
  const int q_lo = blk * 32, q_hi = min(q_lo + 32, nQ);  // this block's queries
  for (int j = q_lo / group + wave; j * group < q_hi; j += DS_W) {  // (uniform over the wave; no barrier below)
    const int row = b * n + j;
    const int t = min(max(pos[row] - plen_raw, 0), slmax - 1);  // the new token's suffix slot; rows 0 .. t - 1 are cached
    const bf16_t* knew = qkv + (long)row * ld + (nq + kvh) * 64;
    const bf16_t* vnew = qkv + (long)row * ld + (nq + nkv + kvh) * 64;
    const bf16_t* skb = sk + (long)row * slmax * w + kvh * 64;
    const bf16_t* svb = sv + (long)row * slmax * w + kvh * 64;
    const int g_lo = max(q_lo - j * group, 0), g_hi = min(q_hi - j * group, group);  // the group's heads in this block
    if (g_lo == 0 && lane < 16) {  // append, by the wave that has the group's first head: 8 lanes x 16 bytes of k, 8 of v
      const int cc = (lane & 7) * 8;
      if (lane < 8) *reinterpret_cast<u32x4*>(sk + ((long)row * slmax + t) * w + kvh * 64 + cc) = *reinterpret_cast<const u32x4*>(knew + cc);
      else *reinterpret_cast<u32x4*>(sv + ((long)row * slmax + t) * w + kvh * 64 + cc) = *reinterpret_cast<const u32x4*>(vnew + cc);
    }
    for (int g0 = g_lo; g0 < g_hi; g0 += DS_H) {
      const int nh = min(DS_H, g_hi - g0);  // (uniform)
      float q[DS_H][8], acc[DS_H][8], m[DS_H], l[DS_H];
#pragma unroll
      for (int h = 0; h < DS_H; ++h) {
        m[h] = -1e30f;
        l[h] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { acc[h][e] = 0.f; q[h][e] = 0.f; }
        if (h < nh) {
          const u32x4 tq = *reinterpret_cast<const u32x4*>(qkv + (long)row * ld + (kvh * group + g0 + h) * 64 + c * 8);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            q[h][2 * e] = from16_lo<F16>(tq[e]) * scale_log2e;
            q[h][2 * e + 1] = from16_hi<F16>(tq[e]) * scale_log2e;
          }
        }
      }
      for (int jb = 0; jb <= t; jb += 64) {
        u32x4 kr[8], vr[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int jj = min(jb + i * 8 + g8, t);
          kr[i] = *reinterpret_cast<const u32x4*>((jj == t ? knew : skb + (long)jj * w) + c * 8);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int jj = min(jb + i * 8 + g8, t);
          vr[i] = *reinterpret_cast<const u32x4*>((jj == t ? vnew : svb + (long)jj * w) + c * 8);
        }
        // scores: a key row is converted once and meets every head's query
        float d[DS_H][8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float kf[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) { kf[2 * e] = from16_lo<F16>(kr[i][e]); kf[2 * e + 1] = from16_hi<F16>(kr[i][e]); }
          const bool live = jb + i * 8 + g8 <= t;
#pragma unroll
          for (int h = 0; h < DS_H; ++h) {
            float x = 0.f;
            if (h < nh) {
#pragma unroll
              for (int e = 0; e < 8; ++e) x = fmaf(q[h][e], kf[e], x);
              x += __shfl_xor(x, 1, 64);
              x += __shfl_xor(x, 2, 64);
              x += __shfl_xor(x, 4, 64);
            }
            d[h][i] = live ? x : -1e30f;
          }
        }
        // per head: the round's maximum, the rescale of what the earlier rounds left, the probabilities (in place of the scores)
#pragma unroll
        for (int h = 0; h < DS_H; ++h) {
          if (h < nh) {
            float rmax = d[h][0];
#pragma unroll
            for (int i = 1; i < 8; ++i) rmax = fmaxf(rmax, d[h][i]);
            rmax = wave_max(rmax);  // (a round holds at least one key: finite)
            const float mnew = fmaxf(m[h], rmax);
            const float alpha = __builtin_amdgcn_exp2f(m[h] - mnew);
            float psum = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[h][e] *= alpha;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              const float p = d[h][i] > -1e29f ? __builtin_amdgcn_exp2f(d[h][i] - mnew) : 0.f;
              psum += p;
              d[h][i] = f16_to_f32(f32_to_f16(p));
            }
            psum = wave_sum(c == 0 ? psum : 0.f);  // (the 8 lanes of a key hold the same p: count it once)
            l[h] = l[h] * alpha + psum;
            m[h] = mnew;
          }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float vf[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) { vf[2 * e] = from16_lo<F16>(vr[i][e]); vf[2 * e + 1] = from16_hi<F16>(vr[i][e]); }
#pragma unroll
          for (int h = 0; h < DS_H; ++h) {
            if (h < nh) {
#pragma unroll
              for (int e = 0; e < 8; ++e) acc[h][e] = fmaf(d[h][i], vf[e], acc[h][e]);
            }
          }
        }
      }
#pragma unroll
      for (int h = 0; h < DS_H; ++h) {
        if (h >= nh) continue;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          acc[h][e] += __shfl_xor(acc[h][e], 8, 64);
          acc[h][e] += __shfl_xor(acc[h][e], 16, 64);
          acc[h][e] += __shfl_xor(acc[h][e], 32, 64);
        }
        if (g8 == 0) {
          const int ql = j * group + g0 + h - q_lo, head = kvh * group + g0 + h;
          const float pm = gstat[0][ql], pl = gstat[1][ql];
          const float M = fmaxf(pm, m[h]);
          const float fpre = __builtin_amdgcn_exp2f(pm - M), fs = __builtin_amdgcn_exp2f(m[h] - M);
          const float inv = 1.f / (pl * fpre + l[h] * fs);  // (> 0: the side that holds M adds at least 1)
          float o[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = (opre[ql * DS_OS + c * 8 + e] * fpre + acc[h][e] * fs) * inv;
          const u32x4 ov = {pack16x2<F16>(o[0], o[1]), pack16x2<F16>(o[2], o[3]), pack16x2<F16>(o[4], o[5]), pack16x2<F16>(o[6], o[7])};
          // (out_frag: the o projection's operand order, common.hpp frag_off: eight consecutive features stay 16 consecutive bytes)
          const long off = out_frag ? frag_off(row, head * 64 + c * 8, nq * 64, out_frag) : (long)row * nq * 64 + head * 64 + c * 8;
          *reinterpret_cast<u32x4*>(out + off) = ov;
        }
      }
    }
  }
}

}  // namespace tcavt

using namespace tcavt;

extern "C" int tcavt_attn_decode_shared(const void* qkv, const void* prefix_k, const void* prefix_v, const int32_t* prefix_len,
                                        void* suffix_k, void* suffix_v, const int32_t* pos, void* out, int B, int n, int nq, int nkv,
                                        int prefix_lmax, int suffix_lmax, float scale, int dtype16, int out_layout,
                                        tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(qkv && prefix_k && prefix_v && prefix_len && suffix_k && suffix_v && pos && out, "attn_decode_shared: null pointer");
  TCAVT_CHECK_ARG(is16(dtype16), "attn_decode_shared: dtype16 must be TCAVT_F16 or TCAVT_BF16");
  TCAVT_CHECK_ARG(B > 0 && nq > 0 && nkv > 0 && nq % nkv == 0 && nq / nkv <= 8,
                  "attn_decode_shared: bad shape (B, nq, nkv > 0, nq %% nkv == 0, nq / nkv <= 8)");
  TCAVT_CHECK_ARG(n >= 1, "attn_decode_shared: n = %d must be >= 1", n);
  TCAVT_CHECK_ARG(prefix_lmax >= 1, "attn_decode_shared: prefix_lmax must be >= 1");
  TCAVT_CHECK_ARG(suffix_lmax >= 1, "attn_decode_shared: suffix_lmax must be >= 1");
  TCAVT_CHECK_ARG(suffix_lmax <= DS_SUFFIX_MAX, "attn_decode_shared: suffix_lmax = %d exceeds TCAVT_ATTN_DECODE_SHARED_MAX_SUFFIX = %d",
                  suffix_lmax, DS_SUFFIX_MAX);
  const long R = (long)B * n;
  const int group = nq / nkv;
  const long nblk = ((long)n * group + 31) / 32;
  TCAVT_CHECK_ARG(R <= 0x7fffffffL && (long)B * nkv * nblk <= 0x7fffffffL, "attn_decode_shared: B * n = %ld rows are too many", R);
  TCAVT_CHECK_ARG(out_layout == 0 || (out_layout == 1 && R <= 32 && (nq * 64) % 256 == 0) || (out_layout == 2 && R <= 8),
                  "attn_decode_shared: out_layout must be 0, 1 (B * n <= 32, nq * 64 %% 256 == 0) or 2 (B * n <= 8)");
  TCAVT_CHECK_ARG(aligned16(qkv) && aligned16(prefix_k) && aligned16(prefix_v) && aligned16(suffix_k) && aligned16(suffix_v) && aligned16(out),
                  "attn_decode_shared: qkv, the prefix, the suffix caches and out must be 16-byte aligned");
  auto kfn = dtype16 == TCAVT_F16 ? attn_decode_shared_kernel<true> : attn_decode_shared_kernel<false>;
  hipLaunchKernelGGL(kfn, dim3((unsigned)(B * nkv * nblk)), dim3(DS_W * 64), 0, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(qkv), static_cast<const bf16_t*>(prefix_k), static_cast<const bf16_t*>(prefix_v), prefix_len,
                     static_cast<bf16_t*>(suffix_k), static_cast<bf16_t*>(suffix_v), pos, static_cast<bf16_t*>(out), n, nq, nkv, prefix_lmax,
                     suffix_lmax, (int)nblk, scale * 1.4426950408889634f, out_layout);
  TCAVT_CHECK_LAUNCH("attn_decode_shared");
  return TCAVT_OK;
}
