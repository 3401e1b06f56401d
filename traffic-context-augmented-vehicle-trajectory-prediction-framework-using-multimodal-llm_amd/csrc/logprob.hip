// Log-probabilities of the generated tokens (tcavt_logprob_begin / tcavt_logprob_finish, include/tcavt.h).
//
// logprob = log_softmax(raw)[token], raw = the fp32 logits row as the lm_head wrote it -- before the repetition penalty, the bans,
// the temperature and top-k / top-p.  The token-selection kernels (csrc/sampler.hip) rewrite the row in place and advance the
// row's state, so two launches bracket them:
//
//   begin   rows x 16 workgroups, before the selection: workgroup (r, g) holds slice g of row r in registers (16-byte loads when the
//           row allows, the same elements through scalar loads otherwise), reduces it to (max, sum exp(x - max)) and records what
//           cannot be known afterwards -- whether the row was live, its step word, its hist_len, and the raw logits at the row's
//           history ids (exactly the elements the repetition penalty may rewrite; a penalised token can still be the one chosen).
//   finish  one wave per row, after the selection: the 16 partials in slice order, the chosen token from out_tokens, its raw logit
//           from the snapshot if the token occurs in the recorded history and from the row otherwise (a banned element is -inf and
//           cannot have been chosen), then (x_tok - M) - log S to token_logprobs, sum_logprob and n_scored.
//
// The summation shape is fixed by V alone: a thread adds its <= 16 elements serially, a wave adds its lanes by xor-butterflies,
// the 16 waves and later the 16 slices are added in index order.  No atomics, no dependence on the logits row, the slot or the
// partner rows: a row's results are bit-identical wherever it runs.  `logits` is only read.
//
// tcavt_logprob_topk (further down) sits between the two: the k most likely tokens of the raw row, from begin's records and partials.
#include "common.hpp"

namespace tcavt {

constexpr int LP_G = 16;     // slices (begin workgroups) per row
constexpr int LP_T = 1024;   // threads per begin workgroup
constexpr int LP_E4 = 4;     // groups of 4 elements a thread holds per round: one round covers V <= 16 * 1024 * 16 = 262 144
constexpr int LP_META = 4;   // int32 per row: live, step, hist_len, slot

struct LogprobP {
  const float* logits;
  const int* slot_of_row;
  const long* history;
  const int* hist_len;
  const int* step;
  const long* out_row;
  const int* finished;
  const long* out_tokens;
  float* token_logprobs;
  float* sum_logprob;
  int* n_scored;
  float* part_m;    // [rows][LP_G]
  float* part_s;    // [rows][LP_G]
  int* meta;        // [rows][LP_META]
  float* raw_hist;  // [rows][hist_cap]
  int rows, V, n_state, hist_cap, out_cap;
};

// workgroup-wide (max, then sum) of one value per thread, the same bits in every thread: lanes by xor-butterflies, waves in
// index order
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();  // (red is reused)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float m = red[0];
#pragma unroll
  for (int w = 1; w < LP_T / 64; ++w) m = fmaxf(m, red[w]);
  return m;
}
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < LP_T / 64; ++w) s += red[w];
  return s;
}

// VEC: the row is 16-byte aligned and V a multiple of 4 -- a group of 4 elements is one 16-byte load.  Otherwise the same groups
// through bounds-checked scalar loads: the arithmetic, and with it every bit of the result, is the same.
template <bool VEC>
__global__ __launch_bounds__(LP_T) void logprob_begin_kernel(LogprobP a) {
  __shared__ float red[LP_T / 64];
  const int r = blockIdx.x / LP_G, g = blockIdx.x % LP_G, tid = threadIdx.x;
  const int s = a.slot_of_row ? a.slot_of_row[r] : r;
  int* meta = a.meta + (long)r * LP_META;
  const bool live = s >= 0 && s < a.n_state && a.finished[s] == 0;  // (uniform)
  if (!live) {
    if (g == 0 && tid == 0) meta[0] = 0;
    return;
  }
  const int V = a.V;
  const int hl = min(max(a.hist_len[s], 0), a.hist_cap);
  if (g == 0 && tid == 0) {
    meta[0] = 1;
    meta[1] = a.out_row ? a.step[s] : a.step[0];
    meta[2] = hl;
    meta[3] = s;
  }
  const float* x = a.logits + (long)r * V;
  // ---- the raw logits at the history ids, the 16 workgroups of the row sharing the entries
  const long* hist = a.history + (long)s * a.hist_cap;
  float* raw = a.raw_hist + (long)r * a.hist_cap;
  for (int i = g * LP_T + tid; i < hl; i += LP_G * LP_T) {
    const long t = hist[i];
    raw[i] = (t >= 0 && t < V) ? x[t] : 0.f;
  }
  // ---- the slice: groups lo4 .. hi4 of 4 elements each (the last group of the row may be short)
  const int n4 = (V + 3) >> 2, chunk4 = (n4 + LP_G - 1) / LP_G;
  const int lo4 = g * chunk4, hi4 = min(lo4 + chunk4, n4);
  float M = -INFINITY, S = 0.f;
  for (int base = lo4; base < hi4; base += LP_E4 * LP_T) {  // one round for V <= 262 144
    f32x4 v[LP_E4];
#pragma unroll
    for (int e = 0; e < LP_E4; ++e) {
      const int i4 = base + tid + e * LP_T;
      f32x4 t = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      if (i4 < hi4) {
        if constexpr (VEC) {
          t = reinterpret_cast<const f32x4*>(x)[i4];
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (4 * i4 + c < V) t[c] = x[4 * i4 + c];
        }
      }
      v[e] = t;
    }
    float m = -INFINITY;
#pragma unroll
    for (int e = 0; e < LP_E4; ++e) m = fmaxf(fmaxf(fmaxf(m, v[e][0]), fmaxf(v[e][1], v[e][2])), v[e][3]);
    const float Mr = block_max(m, red);
    const float sub = Mr == -INFINITY ? 0.f : Mr;  // (an all -inf round adds exp(-inf) = 0, not NaN)
    float acc = 0.f;
#pragma unroll
    for (int e = 0; e < LP_E4; ++e)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc += expf(v[e][c] - sub);  // (a padding -inf adds an exact 0)
    const float Sr = block_sum(acc, red);
    // running (M, S) <- round (Mr, Sr); the first round is taken over exactly: 0 * exp(-inf) + Sr * exp(0)
    const float Mn = fmaxf(M, Mr);
    if (Mn != -INFINITY) S = S * expf(M - Mn) + Sr * expf(Mr - Mn);
    M = Mn;
  }
  if (tid == 0) {
    a.part_m[(long)r * LP_G + g] = M;
    a.part_s[(long)r * LP_G + g] = S;
  }
}

// one wave per row
__global__ __launch_bounds__(64) void logprob_finish_kernel(LogprobP a) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int* meta = a.meta + (long)r * LP_META;
  if (meta[0] == 0) return;  // inert, finished or skipped at the time of the selection (uniform)
  const int step = meta[1], hl = meta[2], s = meta[3];
  if (step < 0 || step >= a.out_cap || s < 0 || s >= a.n_state) return;  // (uniform; the selection wrote no token either)
  const long orow = a.out_row ? a.out_row[s] : (long)r;
  const long tok = a.out_tokens[orow * a.out_cap + step];
  if (tok < 0 || tok >= a.V) return;
  // the token's raw logit: from the snapshot if the token was in the history the selection saw, else the row still holds it
  const long* hist = a.history + (long)s * a.hist_cap;
  const float* raw = a.raw_hist + (long)r * a.hist_cap;
  float snap = -INFINITY;
  bool found = false;
  for (int i = lane; i < hl; i += 64)
    if (hist[i] == tok) {
      found = true;
      snap = raw[i];  // (every occurrence holds the same value)
    }
  const bool any = __any(found);
  snap = wave_max(snap);
  if (lane != 0) return;
  const float xt = any ? snap : a.logits[(long)r * a.V + tok];
  const float* pm = a.part_m + (long)r * LP_G;
  const float* ps = a.part_s + (long)r * LP_G;
  float M = pm[0];
#pragma unroll
  for (int g = 1; g < LP_G; ++g) M = fmaxf(M, pm[g]);
  float S = 0.f;
#pragma unroll
  for (int g = 0; g < LP_G; ++g) S += ps[g] * expf(pm[g] - M);  // (an empty slice is (-inf, 0): adds an exact 0)
  const float lp = (xt - M) - logf(S);
  a.token_logprobs[orow * a.out_cap + step] = lp;
  a.sum_logprob[orow] += lp;  // (one writer per request and launch: plain read-modify-write, in step order)
  a.n_scored[orow] += 1;
}

static inline int64_t lp_align(int64_t n) { return (n + 15) & ~(int64_t)15; }

static int logprob_args(const char* who, const tcavt_logprob_args* a, LogprobP* p) {
  TCAVT_CHECK_ARG(a, "%s: args is a null pointer", who);
  const bool rows = a->slot_of_row != nullptr;
  const struct { const void* p; const char* name; bool need; } ptrs[] = {
      {a->logits, "logits", true}, {a->history, "history", true}, {a->hist_len, "hist_len", true}, {a->step, "step", true},
      {a->out_row, "out_row", rows}, {a->finished, "finished", true}, {a->out_tokens, "out_tokens", true},
      {a->token_logprobs, "token_logprobs", true}, {a->sum_logprob, "sum_logprob", true}, {a->n_scored, "n_scored", true},
      {a->workspace, "workspace", true}};
  for (const auto& q : ptrs) TCAVT_CHECK_ARG(q.p || !q.need, "%s: %s is a null pointer", who, q.name);
  TCAVT_CHECK_ARG(a->rows > 0, "%s: rows = %d must be > 0", who, a->rows);
  TCAVT_CHECK_ARG(a->V > 0, "%s: V = %d must be > 0", who, a->V);
  TCAVT_CHECK_ARG(!rows || a->n_state > 0, "%s: n_state = %d must be > 0 with slot_of_row", who, a->n_state);
  TCAVT_CHECK_ARG(a->hist_cap > 0, "%s: hist_cap = %d must be > 0", who, a->hist_cap);
  TCAVT_CHECK_ARG(a->out_cap > 0, "%s: out_cap = %d must be > 0", who, a->out_cap);
  const int64_t need = tcavt_logprob_workspace_bytes(a->rows, a->hist_cap);
  TCAVT_CHECK_ARG(a->workspace_bytes >= need, "%s: workspace_bytes = %lld, needs %lld", who, (long long)a->workspace_bytes, (long long)need);
  TCAVT_CHECK_ARG(aligned16(a->workspace), "%s: workspace must be 16-byte aligned", who);
  p->logits = a->logits; p->slot_of_row = a->slot_of_row; p->history = reinterpret_cast<const long*>(a->history);
  p->hist_len = a->hist_len; p->step = a->step; p->out_row = reinterpret_cast<const long*>(a->out_row);
  p->finished = a->finished; p->out_tokens = reinterpret_cast<const long*>(a->out_tokens);
  p->token_logprobs = a->token_logprobs; p->sum_logprob = a->sum_logprob; p->n_scored = a->n_scored;
  char* w = static_cast<char*>(a->workspace);
  const int64_t R = a->rows;
  p->part_m = reinterpret_cast<float*>(w); w += lp_align(R * LP_G * 4);
  p->part_s = reinterpret_cast<float*>(w); w += lp_align(R * LP_G * 4);
  p->meta = reinterpret_cast<int*>(w); w += lp_align(R * LP_META * 4);
  p->raw_hist = reinterpret_cast<float*>(w);
  p->rows = a->rows; p->V = a->V; p->n_state = rows ? a->n_state : a->rows; p->hist_cap = a->hist_cap; p->out_cap = a->out_cap;
  return TCAVT_OK;
}

// ---------------------------------------------------------------------------
// tcavt_logprob_topk: the k most likely tokens of the raw row, between begin and the first writer of the logits
// ---------------------------------------------------------------------------
//   slice   rows x 16 workgroups: the slice of logprob_begin again, into registers, then the slice's k first entries by (score
//           descending, id ascending): k rounds of a workgroup-wide arg-max in which only the thread that owned the last winner
//           looks at its registers again (the selection of csrc/beam.hip).  A slice with fewer than k elements pads its list.
//   merge   one wave per row: the 16 * k slice candidates (<= 5 per lane), the same k rounds inside the wave, lane i keeps the
//           i-th winner; (M, log S) from the 16 partials as logprob_finish forms them; (x - M) - log S to top_logprobs.
// The order is decided on the fp32 inputs by comparisons alone, the values by the arithmetic of logprob_finish: a row's lists
// are the same bits wherever it runs.  Both kernels only read the logits and what begin recorded.
constexpr int TK_KMAX = 20;
constexpr int TK_NOKEY = 0x7fffffff;
constexpr int TK_W = LP_T / 64;
constexpr int TK_VMAX = LP_G * LP_T * LP_E4 * 4;                // 262 144: a slice is one round of registers
constexpr int TK_ME = (LP_G * TK_KMAX + 63) / 64;               // slice candidates per lane of the merge: 5

struct TopkP {
  LogprobP lp;
  int* top_ids;    // [n_out][out_cap][k]
  float* top_lp;   // [n_out][out_cap][k]
  float* cand_v;   // [rows][LP_G][k]
  int* cand_k;     // [rows][LP_G][k]: token id, TK_NOKEY = no entry
  int k;
};

__device__ __forceinline__ bool tk_better(float v, int k, float bv, int bk) { return v > bv || (v == bv && k < bk); }
__device__ __forceinline__ bool tk_after(float v, int k, float pv, int pk) { return v < pv || (v == pv && k > pk); }

// the first of a thread's E entries that comes after (pv, pk); pk < 0: the first of all
template <int E>
__device__ __forceinline__ void tk_next(const float (&v)[E], const int (&key)[E], bool any, float pv, int pk, float& bv, int& bk) {
  bv = -INFINITY;
  bk = TK_NOKEY;
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (key[e] != TK_NOKEY && (any || tk_after(v[e], key[e], pv, pk)) && tk_better(v[e], key[e], bv, bk)) { bv = v[e]; bk = key[e]; }
}

// the better of the wave's (v, k) pairs, the same in every lane (the order is total: ids are unique)
__device__ __forceinline__ void tk_wave_best(float& v, int& k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int ok = __shfl_xor(k, o, 64);
    if (tk_better(ov, ok, v, k)) { v = ov; k = ok; }
  }
}

template <bool VEC>
__global__ __launch_bounds__(LP_T) void logprob_topk_slice_kernel(TopkP a) {
  __shared__ float red_v[2][TK_W], out_v[TK_KMAX];
  __shared__ int red_k[2][TK_W], out_k[TK_KMAX];
  const int r = blockIdx.x / LP_G, g = blockIdx.x % LP_G, tid = threadIdx.x;
  if (a.lp.meta[(long)r * LP_META] == 0) return;  // inert, finished or skipped (uniform): nobody reads this row's candidates
  const int V = a.lp.V, K = a.k;
  const float* x = a.lp.logits + (long)r * V;
  const int n4 = (V + 3) >> 2, chunk4 = (n4 + LP_G - 1) / LP_G;
  const int lo4 = g * chunk4, hi4 = min(lo4 + chunk4, n4);
  // ---- the slice in registers (V <= TK_VMAX: one round); an element beyond the slice or the row has no key
  float v[4 * LP_E4];
  int key[4 * LP_E4];
#pragma unroll
  for (int e = 0; e < LP_E4; ++e) {
    const int i4 = lo4 + tid + e * LP_T;
    f32x4 t = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (i4 < hi4) {
      if constexpr (VEC) {
        t = reinterpret_cast<const f32x4*>(x)[i4];
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (4 * i4 + c < V) t[c] = x[4 * i4 + c];
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[4 * e + c] = t[c];
      key[4 * e + c] = (i4 < hi4 && 4 * i4 + c < V) ? 4 * i4 + c : TK_NOKEY;
    }
  }
  // ---- K rounds; red_* alternate, so a round costs one barrier
  const int lane = tid & 63, wv = tid >> 6;
  float bv;
  int bk;
  tk_next(v, key, true, 0.f, 0, bv, bk);
  int cnt = 0;
  for (int k = 0; k < K; ++k) {
    float tv = bv;
    int tk = bk;
    tk_wave_best(tv, tk);
    if (lane == 0) { red_v[k & 1][wv] = tv; red_k[k & 1][wv] = tk; }
    __syncthreads();
    float wvv = red_v[k & 1][0];
    int wk = red_k[k & 1][0];
#pragma unroll
    for (int w = 1; w < TK_W; ++w) {
      const float ov = red_v[k & 1][w];
      const int ok = red_k[k & 1][w];
      if (tk_better(ov, ok, wvv, wk)) { wvv = ov; wk = ok; }
    }
    if (wk == TK_NOKEY) break;  // (uniform) the slice has fewer than K elements
    if (tid == 0) { out_v[k] = wvv; out_k[k] = wk; }
    cnt = k + 1;
    if (bk == wk) tk_next(v, key, false, wvv, wk, bv, bk);  // the owner of the winner: its next entry after it
  }
  __syncthreads();
  if (tid < K) {
    const long o = ((long)r * LP_G + g) * K + tid;
    a.cand_v[o] = tid < cnt ? out_v[tid] : -INFINITY;
    a.cand_k[o] = tid < cnt ? out_k[tid] : TK_NOKEY;
  }
}

// one wave per row
__global__ __launch_bounds__(64) void logprob_topk_merge_kernel(TopkP a) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int* meta = a.lp.meta + (long)r * LP_META;
  if (meta[0] == 0) return;  // (uniform)
  const int step = meta[1], s = meta[3];
  if (step < 0 || step >= a.lp.out_cap || s < 0 || s >= a.lp.n_state) return;  // (uniform; logprob_finish writes nothing either)
  const long orow = a.lp.out_row ? a.lp.out_row[s] : (long)r;
  const int K = a.k, n = LP_G * K;
  const float* cv = a.cand_v + (long)r * n;
  const int* ck = a.cand_k + (long)r * n;
  float v[TK_ME];
  int key[TK_ME];
#pragma unroll
  for (int e = 0; e < TK_ME; ++e) {
    const int q = lane + e * 64;
    v[e] = -INFINITY;
    key[e] = TK_NOKEY;
    if (q < n) {
      v[e] = cv[q];
      key[e] = ck[q];
    }
  }
  float bv, mine_v = -INFINITY;
  int bk, mine_k = TK_NOKEY;
  tk_next(v, key, true, 0.f, 0, bv, bk);
  for (int k = 0; k < K; ++k) {
    float wv = bv;
    int wk = bk;
    tk_wave_best(wv, wk);
    if (wk == TK_NOKEY) break;  // (uniform; K <= V leaves at least K candidates)
    if (lane == k) { mine_v = wv; mine_k = wk; }
    if (bk == wk) tk_next(v, key, false, wv, wk, bv, bk);
  }
  if (lane >= K || mine_k == TK_NOKEY) return;
  // the row's (M, log S): the 16 partials in slice order, as logprob_finish adds them
  const float* pm = a.lp.part_m + (long)r * LP_G;
  const float* ps = a.lp.part_s + (long)r * LP_G;
  float M = pm[0];
#pragma unroll
  for (int g = 1; g < LP_G; ++g) M = fmaxf(M, pm[g]);
  float S = 0.f;
#pragma unroll
  for (int g = 0; g < LP_G; ++g) S += ps[g] * expf(pm[g] - M);
  const long o = (orow * a.lp.out_cap + step) * K + lane;
  a.top_ids[o] = mine_k;
  a.top_lp[o] = (mine_v - M) - logf(S);
}

}  // namespace tcavt

using namespace tcavt;

extern "C" int64_t tcavt_logprob_workspace_bytes(int rows, int hist_cap) {
  if (rows <= 0 || hist_cap <= 0) return 0;
  const int64_t R = rows;
  return 2 * lp_align(R * LP_G * 4) + lp_align(R * LP_META * 4) + lp_align(R * hist_cap * 4);
}

extern "C" int tcavt_logprob_begin(const tcavt_logprob_args* a, tcavt_stream_t stream) {
  LogprobP p;
  const int rc = logprob_args("logprob_begin", a, &p);
  if (rc != TCAVT_OK) return rc;
  const bool vec = (p.V & 3) == 0 && aligned16(p.logits);
  hipLaunchKernelGGL(vec ? logprob_begin_kernel<true> : logprob_begin_kernel<false>, dim3(p.rows * LP_G), dim3(LP_T), 0,
                     static_cast<hipStream_t>(stream), p);
  TCAVT_CHECK_LAUNCH("logprob_begin");
  return TCAVT_OK;
}

extern "C" int tcavt_logprob_finish(const tcavt_logprob_args* a, tcavt_stream_t stream) {
  LogprobP p;
  const int rc = logprob_args("logprob_finish", a, &p);
  if (rc != TCAVT_OK) return rc;
  hipLaunchKernelGGL(logprob_finish_kernel, dim3(p.rows), dim3(64), 0, static_cast<hipStream_t>(stream), p);
  TCAVT_CHECK_LAUNCH("logprob_finish");
  return TCAVT_OK;
}

extern "C" int64_t tcavt_logprob_topk_workspace_bytes(int rows, int k) {
  if (rows <= 0 || k <= 0) return 0;
  return 2 * lp_align((int64_t)rows * LP_G * k * 4);
}

extern "C" int tcavt_logprob_topk(const tcavt_logprob_topk_args* a, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(a, "logprob_topk: args is a null pointer");
  TCAVT_CHECK_ARG(a->lp, "logprob_topk: lp is a null pointer");
  TopkP p;
  const int rc = logprob_args("logprob_topk: lp", a->lp, &p.lp);
  if (rc != TCAVT_OK) return rc;
  TCAVT_CHECK_ARG(a->top_ids, "logprob_topk: top_ids is a null pointer");
  TCAVT_CHECK_ARG(a->top_logprobs, "logprob_topk: top_logprobs is a null pointer");
  TCAVT_CHECK_ARG(a->workspace, "logprob_topk: workspace is a null pointer");
  TCAVT_CHECK_ARG(a->k >= 1 && a->k <= TK_KMAX, "logprob_topk: k = %d must be in [1, %d]", a->k, TK_KMAX);
  TCAVT_CHECK_ARG(a->k <= p.lp.V, "logprob_topk: k = %d must be <= V = %d", a->k, p.lp.V);
  TCAVT_CHECK_ARG(p.lp.V <= TK_VMAX, "logprob_topk: V = %d must be <= %d", p.lp.V, TK_VMAX);
  TCAVT_CHECK_ARG((reinterpret_cast<uintptr_t>(a->top_ids) & 3) == 0, "logprob_topk: top_ids must be 4-byte aligned");
  TCAVT_CHECK_ARG((reinterpret_cast<uintptr_t>(a->top_logprobs) & 3) == 0, "logprob_topk: top_logprobs must be 4-byte aligned");
  const int64_t need = tcavt_logprob_topk_workspace_bytes(p.lp.rows, a->k);
  TCAVT_CHECK_ARG(a->workspace_bytes >= need, "logprob_topk: workspace_bytes = %lld, needs %lld", (long long)a->workspace_bytes, (long long)need);
  TCAVT_CHECK_ARG(aligned16(a->workspace), "logprob_topk: workspace must be 16-byte aligned");
  p.top_ids = a->top_ids; p.top_lp = a->top_logprobs; p.k = a->k;
  char* w = static_cast<char*>(a->workspace);
  p.cand_v = reinterpret_cast<float*>(w); w += lp_align((int64_t)p.lp.rows * LP_G * p.k * 4);
  p.cand_k = reinterpret_cast<int*>(w);
  const bool vec = (p.lp.V & 3) == 0 && aligned16(p.lp.logits);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vec ? logprob_topk_slice_kernel<true> : logprob_topk_slice_kernel<false>, dim3(p.lp.rows * LP_G), dim3(LP_T), 0, st, p);
  hipLaunchKernelGGL(logprob_topk_merge_kernel, dim3(p.lp.rows), dim3(64), 0, st, p);
  TCAVT_CHECK_LAUNCH("logprob_topk");
  return TCAVT_OK;
}
