// Fused lm_head + cross-entropy on labels (HF LlamaForCausalLM with `labels`), forward and backward, for gfx950.
//
//   z = h16[row] . table^T (fp32 accumulation on v_mfma_f32_16x16x32), never stored:
//   forward : per (row, 128-column vocabulary tile) the kernel keeps (max, sum exp) and the target logit; the partials are merged
//             in tile order into lse[row], the per-row loss, the mean loss and the labelled-row count.
//   backward: the logits are recomputed chunk by chunk (LM_CHUNK vocabulary columns), P = exp(z - lse) - onehot goes through the
//             16-bit operand type ONCE (fp16: times 2^14, so that a flat distribution over 128 k tokens stays a normal number;
//             undone exactly at the end), G += P_chunk . table_t_chunk in fp32 in chunk order (tcavt_gemm_bf16, in-place RESIDUAL),
//             and g_out = round16((g_loss / N) * G) on labelled rows, zeros elsewhere.
// Labelled rows are selected and compacted on the device (no host sync): every grid is sized by the upper bound B * L and exits on
// the device count.  No float atomics anywhere: two launches give identical bits.
#include "common.hpp"

namespace tcavt {
namespace {

constexpr int LM_TM = 128;       // rows per workgroup
constexpr int LM_TN = 128;       // vocabulary columns per workgroup
constexpr int LM_BK = 64;        // K elements per LDS stage
constexpr int LM_LDS = LM_BK + 8;  // padded LDS row (elements): 144 bytes, keeps ds_read_b128 of 16 rows off one bank group
constexpr int LM_CHUNK = 16384;  // vocabulary columns of P held at once (backward)
constexpr float LM_P_SCALE_F16 = 16384.f;  // 2^14: |P| <= 1 -> 16384 < 65504; smallest normal P = 2^-28

inline long align_up(long v, long a) { return (v + a - 1) / a * a; }

struct LmLayout {
  long rowidx, tgt, slot, zt, rowloss, part, P, G, total;
  int mcap, ntiles, chunk;
};

LmLayout lm_layout(long rows, int V, int H) {
  LmLayout l;
  l.mcap = (int)align_up(rows, 256);
  l.ntiles = (V + LM_TN - 1) / LM_TN;
  l.chunk = (int)(align_up(V, LM_TN) < LM_CHUNK ? align_up(V, LM_TN) : LM_CHUNK);
  long o = 0;
  l.rowidx = o; o += align_up((long)l.mcap * 4, 256);
  l.tgt = o; o += align_up((long)l.mcap * 4, 256);
  l.slot = o; o += align_up((long)l.mcap * 4, 256);
  l.zt = o; o += align_up((long)l.mcap * 4, 256);
  l.rowloss = o; o += align_up((long)l.mcap * 4, 256);
  l.part = o; o += align_up((long)l.ntiles * l.mcap * 8, 256);
  l.P = o; o += align_up((long)l.mcap * l.chunk * 2, 256);
  l.G = o; o += align_up((long)l.mcap * H * 4, 256);
  l.total = o;
  return l;
}

// the eval pass: the row arrays, the per-tile statistics and the per-tile arg-max (12 bytes per row and tile); no P chunk, no accumulator
struct LmEvalLayout {
  long rowidx, tgt, slot, zt, rowloss, scor, part, amax, total;
  int mcap, ntiles;
};

LmEvalLayout lm_eval_layout(long rows, int V) {
  LmEvalLayout l;
  l.mcap = (int)align_up(rows, 256);
  l.ntiles = (V + LM_TN - 1) / LM_TN;
  long o = 0;
  l.rowidx = o; o += align_up((long)l.mcap * 4, 256);
  l.tgt = o; o += align_up((long)l.mcap * 4, 256);
  l.slot = o; o += align_up((long)l.mcap * 4, 256);
  l.zt = o; o += align_up((long)l.mcap * 4, 256);
  l.rowloss = o; o += align_up((long)l.mcap * 4, 256);
  l.scor = o; o += align_up((long)l.mcap * 4, 256);  // sample_correct when the caller passes none (B <= rows)
  l.part = o; o += align_up((long)l.ntiles * l.mcap * 8, 256);
  l.amax = o; o += align_up((long)l.ntiles * l.mcap * 4, 256);
  l.total = o;
  return l;
}

// ---- labelled-row selection: one workgroup, rows compacted in row order -------------------------------------------------------
__global__ __launch_bounds__(1024) void lm_select_kernel(const int64_t* __restrict__ labels, const int32_t* __restrict__ kv_len, int B, int L,
                                                         int Nq, int V, int mcap, int* __restrict__ rowidx, int* __restrict__ tgt,
                                                         int* __restrict__ slot, int* __restrict__ count, int* __restrict__ flag) {
  __shared__ int s_cnt[1024];
  const int R = B * L, Lt = L - Nq;
  const int per = (R + 1023) / 1024;
  const int r0 = threadIdx.x * per, r1 = min(R, r0 + per);
  auto target_of = [&](int row, bool& bad) -> int {
    const int b = row / L, p = row - b * L;
    if (p >= L - 1 || p + 1 < Nq) return -1;
    const int64_t lab = labels[(long)b * Lt + (p + 1 - Nq)];
    if (lab == -100) return -1;
    if (lab < 0 || lab >= V || (kv_len && p + 1 >= kv_len[b])) { bad = true; return -1; }
    return (int)lab;
  };
  int n = 0;
  bool bad = false;
  for (int r = r0; r < r1; ++r) n += target_of(r, bad) >= 0;
  s_cnt[threadIdx.x] = n;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {  // inclusive scan
    const int v = threadIdx.x >= o ? s_cnt[threadIdx.x - o] : 0;
    __syncthreads();
    s_cnt[threadIdx.x] += v;
    __syncthreads();
  }
  int at = s_cnt[threadIdx.x] - n;
  const int total = s_cnt[1023];
  for (int r = r0; r < r1; ++r) {
    bool b2 = false;
    const int t = target_of(r, b2);
    if (t >= 0) { rowidx[at] = r; tgt[at] = t; slot[r] = at; ++at; }
    else slot[r] = -1;
  }
  for (int r = total + threadIdx.x; r < mcap; r += 1024) { rowidx[r] = 0; tgt[r] = -1; }
  if (threadIdx.x == 0) *count = total;
  if (bad && flag) *flag = 1;
}

// ---- logits tile on MFMA ------------------------------------------------------------------------------------------------------
struct LogitsP {
  const bf16_t* h;  long ldh;
  const bf16_t* table;
  const int* rowidx; const int* tgt; const int* count;
  int V, H, mcap;
  int v0;            // first vocabulary column of this launch (P mode: the chunk's)
  // stats mode
  float2* part; float* zt;
  int* amax;         // MODE 2: [ntiles][mcap] arg-max column of the tile
  // P mode
  const float* lse;  // [B * L], by original row
  bf16_t* P; long ldp;
};

// MODE 0: per-(row, tile) softmax statistics + the target logit.  MODE 1: P = exp(z - lse) - onehot as 16-bit, chunk-local columns.
// MODE 2: MODE 0 plus the tile's arg-max column (after the ragged-tile mask; among equal values the lowest column).
// 4 waves; wave w owns rows 32 w .. 32 w + 31 and all 128 columns.  The table fragment is the MFMA's A operand, so a lane holds
// 4 consecutive vocabulary columns of ONE row: D row (vocab) = 4 (lane >> 4) + reg, D column (row of h) = lane & 15.
template <bool F16, int MODE>
__global__ __launch_bounds__(256) void lm_logits_kernel(LogitsP p) {
  __shared__ __attribute__((aligned(16))) bf16_t s_a[LM_TM * LM_LDS];
  __shared__ __attribute__((aligned(16))) bf16_t s_b[LM_TN * LM_LDS];
  const int n = *p.count;
  const int m_base = blockIdx.x * LM_TM;
  const int tile = blockIdx.y;
  const int vt = p.v0 + tile * LM_TN;  // first vocabulary column of this tile
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (m_base >= n) {
    if constexpr (MODE == 1) {  // rows beyond the count feed the chunk GEMM: zeros
      for (int e = tid; e < LM_TM * (LM_TN / 8); e += 256) {
        const int r = e / (LM_TN / 8), c = e % (LM_TN / 8);
        *reinterpret_cast<u32x4*>(p.P + (long)(m_base + r) * p.ldp + tile * LM_TN + c * 8) = u32x4{0, 0, 0, 0};
      }
    }
    return;
  }

  // staging: thread handles vectors (row = tid / 8 + 32 i, 16-byte piece tid % 8), i = 0..3, of both operands
  const int srow = tid >> 3, spc = tid & 7;
  const bf16_t* ga[4];
  const bf16_t* gb[4];
  bool bok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = m_base + srow + 32 * i;  // < mcap; rowidx is 0 beyond the count
    ga[i] = p.h + (long)p.rowidx[r] * p.ldh + spc * 8;
    const int v = vt + srow + 32 * i;
    bok[i] = v < p.V;
    gb[i] = p.table + (long)(bok[i] ? v : 0) * p.H + spc * 8;
  }
  u32x4 ra[4], rb[4];
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = *reinterpret_cast<const u32x4*>(ga[i] + k0);
      rb[i] = bok[i] ? *reinterpret_cast<const u32x4*>(gb[i] + k0) : u32x4{0, 0, 0, 0};
    }
  };
  f32x4 acc[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  gload(0);
  for (int k0 = 0; k0 < p.H; k0 += LM_BK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<u32x4*>(&s_a[(srow + 32 * i) * LM_LDS + spc * 8]) = ra[i];
      *reinterpret_cast<u32x4*>(&s_b[(srow + 32 * i) * LM_LDS + spc * 8]) = rb[i];
    }
    __syncthreads();
    if (k0 + LM_BK < p.H) gload(k0 + LM_BK);
#pragma unroll
    for (int ks = 0; ks < LM_BK / 32; ++ks) {
      u32x4 af[2], bf[8];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const u32x4*>(&s_a[(32 * w + 16 * i + fr) * LM_LDS + ks * 32 + fq * 8]);
#pragma unroll
      for (int j = 0; j < 8; ++j) bf[j] = *reinterpret_cast<const u32x4*>(&s_b[(16 * j + fr) * LM_LDS + ks * 32 + fq * 8]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if constexpr (F16)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, bf[j]), __builtin_bit_cast(f16x8, af[i]), acc[i][j], 0, 0, 0);
          else
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bf[j]), __builtin_bit_cast(bf16x8, af[i]), acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();
  }

  // lane: row m_base + 32 w + 16 i + fr, columns vt + 16 j + 4 fq + e
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = m_base + 32 * w + 16 * i + fr;
    const bool live = r < n;
    const int t = p.tgt[r];  // -1 beyond the count
    if constexpr (MODE == 0 || MODE == 2) {
      float mx = -INFINITY;
      [[maybe_unused]] float bv = -INFINITY;  // MODE 2: greatest value so far and its column; columns are visited in rising order,
      [[maybe_unused]] int bi = 0x7fffffff;     // so a strict > keeps the lowest column among equal values
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int v = vt + 16 * j + 4 * fq + e;
          if (v >= p.V) acc[i][j][e] = -INFINITY;  // ragged last tile: masked, never padded with zeros
          mx = fmaxf(mx, acc[i][j][e]);
          if constexpr (MODE == 2) {
            if (acc[i][j][e] > bv) { bv = acc[i][j][e]; bi = v; }
          }
          if (live && v == t) p.zt[r] = acc[i][j][e];  // exactly one lane of one tile owns column t
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      if constexpr (MODE == 2) {  // the index travels with the value: greater value first, lower column on equality
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
          const float ov = __shfl_xor(bv, o, 64);
          const int oi = __shfl_xor(bi, o, 64);
          if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (live && fq == 0) p.amax[(long)tile * p.mcap + r] = bi;
      }
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) s += expf(acc[i][j][e] - mx);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (live && fq == 0) p.part[(long)(p.v0 / LM_TN + tile) * p.mcap + r] = make_float2(mx, s);
    } else {
      const float lse = live ? p.lse[p.rowidx[r]] : 0.f;
      constexpr float sc = F16 ? LM_P_SCALE_F16 : 1.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float pv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int v = vt + 16 * j + 4 * fq + e;
          float q = expf(acc[i][j][e] - lse) - (v == t ? 1.f : 0.f);
          if (!live || v >= p.V) q = 0.f;
          pv[e] = q * sc;
        }
        u32x2 o{pack16x2<F16>(pv[0], pv[1]), pack16x2<F16>(pv[2], pv[3])};
        *reinterpret_cast<u32x2*>(p.P + (long)r * p.ldp + tile * LM_TN + 16 * j + 4 * fq) = o;
      }
    }
  }
}

// ---- merge of the per-tile statistics, in tile order ----------------------------------------------------------------------------
// EVAL: also the row's arg-max -- that of the tile with the greatest maximum, the lowest tile among equal maxima.  The
// (max, sum exp) arithmetic is the same code in both instantiations.
template <bool EVAL>
__global__ __launch_bounds__(256) void lm_merge_kernel(const float2* __restrict__ part, const float* __restrict__ zt, const int* __restrict__ rowidx,
                                                       const int* __restrict__ count, int ntiles, int mcap, float* __restrict__ lse,
                                                       float* __restrict__ row_loss, float* __restrict__ rowloss_c,
                                                       const int* __restrict__ amax, int* __restrict__ pred) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= *count) return;
  float mx = -INFINITY;
  [[maybe_unused]] int bt = 0;
  for (int t = 0; t < ntiles; ++t) {
    const float x = part[(long)t * mcap + r].x;
    if constexpr (EVAL) {
      if (x > mx) bt = t;  // strict: the lowest tile keeps an equal maximum
    }
    mx = fmaxf(mx, x);
  }
  if constexpr (EVAL) pred[rowidx[r]] = amax[(long)bt * mcap + r];
  float s = 0.f;
  for (int t = 0; t < ntiles; ++t) {
    const float2 q = part[(long)t * mcap + r];
    s += q.y * expf(q.x - mx);
  }
  const float ls = logf(s);
  const float l = mx + ls;
  const float rl = (mx - zt[r]) + ls;  // not l - z[t]: with large logits l is rounded at ulp(|z|), the difference mx - z[t] is not
  const int o = rowidx[r];
  lse[o] = l;
  if (row_loss) row_loss[o] = rl;
  rowloss_c[r] = rl;
}

// unlabelled rows of lse / row_loss read zero
__global__ __launch_bounds__(256) void lm_clear_rows_kernel(const int* __restrict__ slot, int R, float* __restrict__ lse, float* __restrict__ row_loss) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < R && slot[r] < 0) {
    lse[r] = 0.f;
    if (row_loss) row_loss[r] = 0.f;
  }
}

// unlabelled rows of pred read -1
__global__ __launch_bounds__(256) void lm_clear_pred_kernel(const int* __restrict__ slot, int R, int* __restrict__ pred) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < R && slot[r] < 0) pred[r] = -1;
}

// per-sample sums: workgroup b walks the rows of sample b, thread t rows t, t + 256, ...; LDS tree.  Fixed order, fp64 partial sums.
__global__ __launch_bounds__(256) void lm_sample_kernel(const int* __restrict__ slot, const int* __restrict__ tgt, const float* __restrict__ rowloss_c,
                                                        const int* __restrict__ pred, int L, int* __restrict__ sample_tokens,
                                                        int* __restrict__ sample_correct, float* __restrict__ sample_nll) {
  __shared__ double s_sum[256];
  __shared__ int s_tok[256], s_cor[256];
  const int b = blockIdx.x;
  double a = 0.0;
  int nt = 0, nc = 0;
  for (int p = threadIdx.x; p < L; p += 256) {
    const int r = b * L + p, s = slot[r];
    if (s >= 0) {
      a += (double)rowloss_c[s];
      ++nt;
      nc += pred[r] == tgt[s];
    }
  }
  s_sum[threadIdx.x] = a; s_tok[threadIdx.x] = nt; s_cor[threadIdx.x] = nc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
      s_tok[threadIdx.x] += s_tok[threadIdx.x + o];
      s_cor[threadIdx.x] += s_cor[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (sample_tokens) sample_tokens[b] = s_tok[0];
    sample_correct[b] = s_cor[0];
    if (sample_nll) sample_nll[b] = (float)s_sum[0];
  }
}

// correct = sum of sample_correct: one workgroup
__global__ __launch_bounds__(256) void lm_correct_kernel(const int* __restrict__ sample_correct, int B, int* __restrict__ correct) {
  __shared__ int s_cor[256];
  int n = 0;
  for (int b = threadIdx.x; b < B; b += 256) n += sample_correct[b];
  s_cor[threadIdx.x] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_cor[threadIdx.x] += s_cor[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *correct = s_cor[0];
}

// mean over the labelled rows: one workgroup, fixed order, fp64 partial sums.  N = 0: 0 / 0 = NaN, as torch gives.
__global__ __launch_bounds__(256) void lm_mean_kernel(const float* __restrict__ rowloss_c, const int* __restrict__ count, float* __restrict__ loss) {
  __shared__ double s_sum[256];
  const int n = *count;
  double a = 0.0;
  for (int r = threadIdx.x; r < n; r += 256) a += (double)rowloss_c[r];
  s_sum[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (float)(s_sum[0] / (double)n);
}

// g_out[row] = round16(scale * G[slot[row]]) on labelled rows, zeros elsewhere; scale = (g_loss / N) * unscale in fp32
template <bool OUT_F16>
__global__ __launch_bounds__(256) void lm_scatter_kernel(const float* __restrict__ G, const int* __restrict__ slot, const int* __restrict__ count,
                                                         const float* __restrict__ g_loss, float unscale, int R, int H, bf16_t* __restrict__ out,
                                                         long ldg) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const int per = H / 4;
  if (e >= (long)R * per) return;
  const int r = (int)(e / per), c = (int)(e % per) * 4;
  const int s = slot[r];
  u32x2 o{0u, 0u};
  if (s >= 0) {
    const float sc = ((g_loss ? *g_loss : 1.f) / (float)*count) * unscale;
    const f32x4 g = *reinterpret_cast<const f32x4*>(G + (long)s * H + c);
    o = u32x2{pack16x2<OUT_F16>(g[0] * sc, g[1] * sc), pack16x2<OUT_F16>(g[2] * sc, g[3] * sc)};
  }
  *reinterpret_cast<u32x2*>(out + (long)r * ldg + c) = o;
}

int lm_check_common(const tcavt_lm_loss_args* a, const char* who, LmLayout* lay) {
  TCAVT_CHECK_ARG(a != nullptr, "%s: null args", who);
  TCAVT_CHECK_ARG(a->h16 && a->table && a->labels && a->count && a->lse && a->workspace, "%s: null h16 / table / labels / count / lse / workspace", who);
  TCAVT_CHECK_ARG(a->B > 0 && a->L > 1 && a->Nq >= 0 && a->Nq < a->L, "%s: bad B / L / Nq %d / %d / %d", who, a->B, a->L, a->Nq);
  TCAVT_CHECK_ARG((long)a->B * a->L < (1 << 24), "%s: B * L too large", who);
  TCAVT_CHECK_ARG(a->V > 0 && a->V % 16 == 0, "%s: V=%d must be a multiple of 16", who, a->V);
  TCAVT_CHECK_ARG(a->H > 0 && a->H % 256 == 0, "%s: H=%d must be a multiple of 256", who, a->H);
  TCAVT_CHECK_ARG(a->dtype16 == TCAVT_BF16 || a->dtype16 == TCAVT_F16, "%s: dtype16 must be TCAVT_BF16 or TCAVT_F16", who);
  TCAVT_CHECK_ARG(a->ldh >= a->H && a->ldh % 8 == 0 && aligned16(a->h16) && aligned16(a->table), "%s: h16 / table need 16-byte alignment, ldh >= H and %% 8 == 0", who);
  *lay = lm_layout((long)a->B * a->L, a->V, a->H);
  TCAVT_CHECK_ARG(a->workspace_bytes >= lay->total, "%s: workspace too small: %ld bytes, need %ld (tcavt_lm_loss_workspace_bytes)", who,
                  (long)a->workspace_bytes, lay->total);
  TCAVT_CHECK_ARG(((uintptr_t)a->workspace & 255) == 0, "%s: workspace must be 256-byte aligned", who);
  return TCAVT_OK;
}

int lm_select(const tcavt_lm_loss_args* a, const LmLayout& lay, hipStream_t s) {
  char* ws = static_cast<char*>(a->workspace);
  hipLaunchKernelGGL(lm_select_kernel, dim3(1), dim3(1024), 0, s, a->labels, a->kv_len, a->B, a->L, a->Nq, a->V, lay.mcap,
                     reinterpret_cast<int*>(ws + lay.rowidx), reinterpret_cast<int*>(ws + lay.tgt), reinterpret_cast<int*>(ws + lay.slot), a->count,
                     a->flag);
  TCAVT_CHECK_LAUNCH("lm_loss(select)");
  return TCAVT_OK;
}

LogitsP lm_logits_params(const tcavt_lm_loss_args* a, const LmLayout& lay) {
  char* ws = static_cast<char*>(a->workspace);
  LogitsP p;
  p.h = static_cast<const bf16_t*>(a->h16); p.ldh = a->ldh;
  p.table = static_cast<const bf16_t*>(a->table);
  p.rowidx = reinterpret_cast<const int*>(ws + lay.rowidx);
  p.tgt = reinterpret_cast<const int*>(ws + lay.tgt);
  p.count = a->count;
  p.V = a->V; p.H = a->H; p.mcap = lay.mcap; p.v0 = 0;
  p.part = reinterpret_cast<float2*>(ws + lay.part);
  p.zt = reinterpret_cast<float*>(ws + lay.zt);
  p.amax = nullptr;
  p.lse = a->lse;
  p.P = reinterpret_cast<bf16_t*>(ws + lay.P); p.ldp = lay.chunk;
  return p;
}

}  // namespace
}  // namespace tcavt

using namespace tcavt;

extern "C" int64_t tcavt_lm_loss_workspace_bytes(int64_t rows, int V, int H) {
  if (rows <= 0 || V <= 0 || H <= 0) return 0;
  return lm_layout(rows, V, H).total;
}

extern "C" int tcavt_lm_loss_forward(const tcavt_lm_loss_args* a, tcavt_stream_t stream) {
  LmLayout lay;
  if (int rc = lm_check_common(a, "lm_loss_forward", &lay)) return rc;
  TCAVT_CHECK_ARG(a->loss != nullptr, "lm_loss_forward: null loss");
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(a->workspace);
  const int R = a->B * a->L;
  if (int rc = lm_select(a, lay, s)) return rc;
  LogitsP p = lm_logits_params(a, lay);
  const dim3 grid(lay.mcap / LM_TM, lay.ntiles);
  if (a->dtype16 == TCAVT_F16) hipLaunchKernelGGL((lm_logits_kernel<true, 0>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((lm_logits_kernel<false, 0>), grid, dim3(256), 0, s, p);
  TCAVT_CHECK_LAUNCH("lm_loss_forward(logits)");
  hipLaunchKernelGGL(lm_clear_rows_kernel, dim3((R + 255) / 256), dim3(256), 0, s, reinterpret_cast<const int*>(ws + lay.slot), R, a->lse, a->row_loss);
  hipLaunchKernelGGL(lm_merge_kernel<false>, dim3(lay.mcap / 256), dim3(256), 0, s, p.part, p.zt, p.rowidx, a->count, lay.ntiles, lay.mcap, a->lse,
                     a->row_loss, reinterpret_cast<float*>(ws + lay.rowloss), nullptr, nullptr);
  hipLaunchKernelGGL(lm_mean_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<const float*>(ws + lay.rowloss), a->count, a->loss);
  TCAVT_CHECK_LAUNCH("lm_loss_forward(merge)");
  return TCAVT_OK;
}

extern "C" int tcavt_lm_loss_backward(const tcavt_lm_loss_args* a, tcavt_stream_t stream) {
  LmLayout lay;
  if (int rc = lm_check_common(a, "lm_loss_backward", &lay)) return rc;
  TCAVT_CHECK_ARG(a->g_out && aligned16(a->g_out) && a->ldg >= a->H && a->ldg % 4 == 0, "lm_loss_backward: g_out needs 16-byte alignment, ldg >= H and %% 4 == 0");
  TCAVT_CHECK_ARG(a->grad_dtype == TCAVT_BF16 || a->grad_dtype == TCAVT_F16, "lm_loss_backward: grad_dtype must be TCAVT_BF16 or TCAVT_F16");
  const long vpad = align_up(a->V, 64);
  TCAVT_CHECK_ARG(a->table_t && aligned16(a->table_t) && a->ldt >= vpad && a->ldt % 8 == 0,
                  "lm_loss_backward: needs table_t, the 16-bit transpose [H][ldt] of the table with ldt >= V rounded up to 64 (zero-filled beyond V) and %% 8 == 0");
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(a->workspace);
  const int R = a->B * a->L;
  const bool f16 = a->dtype16 == TCAVT_F16;
  if (int rc = lm_select(a, lay, s)) return rc;
  LogitsP p = lm_logits_params(a, lay);
  float* G = reinterpret_cast<float*>(ws + lay.G);
  for (int v0 = 0; v0 < a->V; v0 += lay.chunk) {  // fixed chunk order: bit-reproducible
    const int width = a->V - v0 < lay.chunk ? a->V - v0 : lay.chunk;
    p.v0 = v0;
    const dim3 grid(lay.mcap / LM_TM, (width + LM_TN - 1) / LM_TN);
    if (f16) hipLaunchKernelGGL((lm_logits_kernel<true, 1>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((lm_logits_kernel<false, 1>), grid, dim3(256), 0, s, p);
    TCAVT_CHECK_LAUNCH("lm_loss_backward(P)");
    tcavt_gemm_args g = {};
    g.A = p.P; g.lda = lay.chunk;
    g.W = static_cast<const bf16_t*>(a->table_t) + v0; g.ldw = a->ldt;
    g.C = G; g.ldc = a->H;
    g.M = lay.mcap; g.N = a->H; g.K = (int)align_up(width, 64);
    g.out_dtype = TCAVT_F32;
    g.in_dtype = a->dtype16;
    if (v0 > 0) { g.epilogue = TCAVT_EPI_RESIDUAL; g.residual = G; g.ldr = a->H; }  // in place: G += P_chunk . table_t_chunk
    if (int rc = tcavt_gemm_bf16(&g, stream)) return rc;
  }
  const float unscale = f16 ? 1.f / LM_P_SCALE_F16 : 1.f;
  const long threads = (long)R * (a->H / 4);
  const dim3 sg((unsigned)((threads + 255) / 256));
  const int* slot = reinterpret_cast<const int*>(ws + lay.slot);
  if (a->grad_dtype == TCAVT_F16)
    hipLaunchKernelGGL(lm_scatter_kernel<true>, sg, dim3(256), 0, s, G, slot, a->count, a->g_loss, unscale, R, a->H, static_cast<bf16_t*>(a->g_out), (long)a->ldg);
  else
    hipLaunchKernelGGL(lm_scatter_kernel<false>, sg, dim3(256), 0, s, G, slot, a->count, a->g_loss, unscale, R, a->H, static_cast<bf16_t*>(a->g_out), (long)a->ldg);
  TCAVT_CHECK_LAUNCH("lm_loss_backward(scatter)");
  return TCAVT_OK;
}

extern "C" int64_t tcavt_lm_eval_workspace_bytes(int64_t rows, int V, int H) {
  if (rows <= 0 || V <= 0 || H <= 0) return 0;
  return lm_eval_layout(rows, V).total;
}

extern "C" int tcavt_lm_eval(const tcavt_lm_eval_args* a, tcavt_stream_t stream) {
  const char* who = "lm_eval";
  TCAVT_CHECK_ARG(a != nullptr, "%s: null args", who);
  TCAVT_CHECK_ARG(a->h16 && a->table && a->labels && a->count && a->lse && a->workspace, "%s: null h16 / table / labels / count / lse / workspace", who);
  TCAVT_CHECK_ARG(a->loss != nullptr, "%s: null loss", who);
  TCAVT_CHECK_ARG(a->pred != nullptr, "%s: null pred", who);
  TCAVT_CHECK_ARG(a->B > 0 && a->L > 1 && a->Nq >= 0 && a->Nq < a->L, "%s: bad B / L / Nq %d / %d / %d", who, a->B, a->L, a->Nq);
  TCAVT_CHECK_ARG((long)a->B * a->L < (1 << 24), "%s: B * L too large", who);
  TCAVT_CHECK_ARG(a->V > 0 && a->V % 16 == 0, "%s: V=%d must be a multiple of 16", who, a->V);
  TCAVT_CHECK_ARG(a->H > 0 && a->H % 256 == 0, "%s: H=%d must be a multiple of 256", who, a->H);
  TCAVT_CHECK_ARG(a->dtype16 == TCAVT_BF16 || a->dtype16 == TCAVT_F16, "%s: dtype16 must be TCAVT_BF16 or TCAVT_F16", who);
  TCAVT_CHECK_ARG(a->ldh >= a->H && a->ldh % 8 == 0 && aligned16(a->h16) && aligned16(a->table), "%s: h16 / table need 16-byte alignment, ldh >= H and %% 8 == 0", who);
  const LmEvalLayout lay = lm_eval_layout((long)a->B * a->L, a->V);
  TCAVT_CHECK_ARG(a->workspace_bytes >= lay.total, "%s: workspace too small: %ld bytes, need %ld (tcavt_lm_eval_workspace_bytes)", who,
                  (long)a->workspace_bytes, lay.total);
  TCAVT_CHECK_ARG(((uintptr_t)a->workspace & 255) == 0, "%s: workspace must be 256-byte aligned", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(a->workspace);
  const int R = a->B * a->L;
  int* rowidx = reinterpret_cast<int*>(ws + lay.rowidx);
  int* tgt = reinterpret_cast<int*>(ws + lay.tgt);
  int* slot = reinterpret_cast<int*>(ws + lay.slot);
  float* rowloss_c = reinterpret_cast<float*>(ws + lay.rowloss);
  int* scor = a->sample_correct ? a->sample_correct : reinterpret_cast<int*>(ws + lay.scor);
  hipLaunchKernelGGL(lm_select_kernel, dim3(1), dim3(1024), 0, s, a->labels, a->kv_len, a->B, a->L, a->Nq, a->V, lay.mcap, rowidx, tgt, slot, a->count,
                     a->flag);
  TCAVT_CHECK_LAUNCH("lm_eval(select)");
  LogitsP p;
  p.h = static_cast<const bf16_t*>(a->h16); p.ldh = a->ldh;
  p.table = static_cast<const bf16_t*>(a->table);
  p.rowidx = rowidx; p.tgt = tgt; p.count = a->count;
  p.V = a->V; p.H = a->H; p.mcap = lay.mcap; p.v0 = 0;
  p.part = reinterpret_cast<float2*>(ws + lay.part);
  p.zt = reinterpret_cast<float*>(ws + lay.zt);
  p.amax = reinterpret_cast<int*>(ws + lay.amax);
  p.lse = nullptr; p.P = nullptr; p.ldp = 0;
  const dim3 grid(lay.mcap / LM_TM, lay.ntiles);
  if (a->dtype16 == TCAVT_F16) hipLaunchKernelGGL((lm_logits_kernel<true, 2>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((lm_logits_kernel<false, 2>), grid, dim3(256), 0, s, p);
  TCAVT_CHECK_LAUNCH("lm_eval(logits)");
  hipLaunchKernelGGL(lm_clear_rows_kernel, dim3((R + 255) / 256), dim3(256), 0, s, slot, R, a->lse, a->row_loss);
  hipLaunchKernelGGL(lm_clear_pred_kernel, dim3((R + 255) / 256), dim3(256), 0, s, slot, R, a->pred);
  hipLaunchKernelGGL(lm_merge_kernel<true>, dim3(lay.mcap / 256), dim3(256), 0, s, p.part, p.zt, p.rowidx, a->count, lay.ntiles, lay.mcap, a->lse,
                     a->row_loss, rowloss_c, p.amax, a->pred);
  hipLaunchKernelGGL(lm_mean_kernel, dim3(1), dim3(256), 0, s, rowloss_c, a->count, a->loss);
  TCAVT_CHECK_LAUNCH("lm_eval(merge)");
  hipLaunchKernelGGL(lm_sample_kernel, dim3(a->B), dim3(256), 0, s, slot, tgt, rowloss_c, a->pred, a->L, a->sample_tokens, scor, a->sample_nll);
  if (a->correct) hipLaunchKernelGGL(lm_correct_kernel, dim3(1), dim3(256), 0, s, scor, a->B, a->correct);
  TCAVT_CHECK_LAUNCH("lm_eval(samples)");
  return TCAVT_OK;
}
