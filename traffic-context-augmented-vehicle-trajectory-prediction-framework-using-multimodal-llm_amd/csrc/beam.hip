// Beam search of text generation (include/tcavt.h: tcavt_beam_select, tcavt_beam_reorder, tcavt_beam_workspace_bytes; DESIGN.md
// section 7).  R = B * n decode rows, n beams per prompt (row r = b * n + j), K = 2 n candidates per prompt and step.
//
// tcavt_beam_select is three launches on one stream:
//   partial  R x 16 workgroups: (max, sum exp(x - max)) of slice g of every live row -- the reduction of csrc/logprob.hip, element
//            for element and in its order, so the summation shape depends on V alone.
//   slice    R x 16 workgroups: the 16 partials of the row in slice order -> (M, log S); the slice's elements again, into registers:
//            lp = (x - M) - log S, the processors ON lp (a byte map of the slice in LDS says which tokens the history penalises or
//            bans), acc = lp + run_score; then the slice's K best (acc descending, token ascending) by K rounds of a workgroup-wide
//            arg-max in which only the thread that owned the last winner looks at its registers again.
//   merge    one workgroup per prompt: the n * 16 * K slice candidates, the same K rounds, then the bookkeeping of the step (new
//            running beams, the finished store, the early-stop heuristic, the done flag) and the plan of the reorder.
// tcavt_beam_reorder is one launch: a thread owns one 16-byte piece position (k or v, layer, prompt, suffix slot, piece), loads it
// from every row that is somebody's parent and stores it to every row whose parent is another row -- in place, no second buffer;
// behind those, one workgroup per prompt moves the generated part of the histories the same way, appends the new tokens and
// advances hist_len, pos and the prompt's step word.
// The logits are only read.  No atomics; nothing depends on another prompt, so a prompt's results are the same bits beside any other.
#include "common.hpp"

namespace tcavt {

constexpr int BM_G = 16;      // slices per row (= LP_G of csrc/logprob.hip)
constexpr int BM_T = 1024;    // threads of a select workgroup (= LP_T)
constexpr int BM_E4 = 4;      // groups of 4 elements per thread: a slice of up to 4 * 1024 * 4 elements in ONE round
constexpr int BM_NMAX = 16;   // beams per prompt
constexpr int BM_KMAX = 2 * BM_NMAX;
constexpr int BM_VMAX = BM_G * BM_T * BM_E4 * 4;  // 262 144
constexpr int BM_SLICE = BM_T * BM_E4 * 4;        // elements of a slice at most
constexpr int BM_NOKEY = 0x7fffffff;
constexpr int BM_W = BM_T / 64;

struct BeamP {
  const float* logits;
  const long* history;
  const int* hist_len;
  float* run_score;
  int* live;
  long* fin_tokens;
  float* fin_score;
  int* fin_flag;
  int* fin_len;
  int* unsat;
  int* done;
  long* cur_tok;
  const int* pos;
  int* finished;
  const int* step;
  const int* prefix_len;
  const float* len_pow;
  int* parent;
  int* plan;
  int* trace;
  float* part_m;  // [R][BM_G]
  float* part_s;  // [R][BM_G]
  int* cand_n;    // [R][BM_G]
  float* cand_v;  // [R][BM_G][BM_KMAX]
  int* cand_k;    // [R][BM_G][BM_KMAX]: key = j * V + token
  long eos, pad;
  float penalty;
  int ngram, early, R, n, V, N, hist_cap;
};

__device__ __forceinline__ bool bm_after(float v, int k, float pv, int pk) { return v < pv || (v == pv && k > pk); }
__device__ __forceinline__ bool bm_better(float v, int k, float bv, int bk) { return v > bv || (v == bv && k < bk); }

__device__ __forceinline__ float bm_block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float m = red[0];
#pragma unroll
  for (int w = 1; w < BM_W; ++w) m = fmaxf(m, red[w]);
  return m;
}
__device__ __forceinline__ float bm_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < BM_W; ++w) s += red[w];
  return s;
}

// groups lo4 .. hi4 of 4 elements: slice g of a row of V elements (the cut of logprob_begin)
__device__ __forceinline__ void bm_slice(int V, int g, int& lo4, int& hi4) {
  const int n4 = (V + 3) >> 2, chunk4 = (n4 + BM_G - 1) / BM_G;
  lo4 = g * chunk4;
  hi4 = min(lo4 + chunk4, n4);
}

// group i4 of the row: one 16-byte load (VEC: row 16-byte aligned, V % 4 == 0) or four bounded scalar loads; -inf beyond the row
template <bool VEC>
__device__ __forceinline__ f32x4 bm_load4(const float* x, int i4, int hi4, int V) {
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
  return t;
}

template <bool VEC>
__global__ __launch_bounds__(BM_T) void beam_partial_kernel(BeamP a) {
  __shared__ float red[BM_W];
  const int r = blockIdx.x / BM_G, g = blockIdx.x % BM_G, tid = threadIdx.x;
  if (a.done[r / a.n] != 0 || a.live[r] == 0) return;  // (uniform; nobody reads this row's partials)
  const int V = a.V;
  const float* x = a.logits + (long)r * V;
  int lo4, hi4;
  bm_slice(V, g, lo4, hi4);
  f32x4 v[BM_E4];
#pragma unroll
  for (int e = 0; e < BM_E4; ++e) v[e] = bm_load4<VEC>(x, lo4 + tid + e * BM_T, hi4, V);
  float m = -INFINITY;
#pragma unroll
  for (int e = 0; e < BM_E4; ++e) m = fmaxf(fmaxf(fmaxf(m, v[e][0]), fmaxf(v[e][1], v[e][2])), v[e][3]);
  const float Mr = bm_block_max(m, red);
  const float sub = Mr == -INFINITY ? 0.f : Mr;
  float acc = 0.f;
#pragma unroll
  for (int e = 0; e < BM_E4; ++e)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc += expf(v[e][c] - sub);
  const float Sr = bm_block_sum(acc, red);
  if (tid == 0) {
    a.part_m[(long)r * BM_G + g] = Mr;
    a.part_s[(long)r * BM_G + g] = Sr;
  }
}

// The K first of the workgroup's E entries per thread in (value descending, key ascending) order -> out_v / out_k (LDS, K entries),
// returns how many exist (entries with key BM_NOKEY do not).  Every thread of the workgroup calls it; red_* are two buffers that
// alternate, so a round costs one barrier.
template <int E>
__device__ __forceinline__ int bm_block_topk(const float (&v)[E], const int (&key)[E], int K, float* out_v, int* out_k,
                                             float (*red_v)[BM_W], int (*red_k)[BM_W]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float bv = -INFINITY;
  int bk = BM_NOKEY;
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (key[e] != BM_NOKEY && bm_better(v[e], key[e], bv, bk)) { bv = v[e]; bk = key[e]; }
  int cnt = 0;
  for (int k = 0; k < K; ++k) {
    float tv = bv;
    int tk = bk;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(tv, o, 64);
      const int ok = __shfl_xor(tk, o, 64);
      if (bm_better(ov, ok, tv, tk)) { tv = ov; tk = ok; }
    }
    if (lane == 0) { red_v[k & 1][wv] = tv; red_k[k & 1][wv] = tk; }
    __syncthreads();
    float wvv = red_v[k & 1][0];
    int wk = red_k[k & 1][0];
#pragma unroll
    for (int w = 1; w < BM_W; ++w) {
      const float ov = red_v[k & 1][w];
      const int ok = red_k[k & 1][w];
      if (bm_better(ov, ok, wvv, wk)) { wvv = ov; wk = ok; }
    }
    if (wk == BM_NOKEY) break;  // (uniform)
    if (threadIdx.x == 0) { out_v[k] = wvv; out_k[k] = wk; }
    cnt = k + 1;
    if (bk == wk) {  // the owner of the winner: its next entry after it
      bv = -INFINITY;
      bk = BM_NOKEY;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (key[e] != BM_NOKEY && bm_after(v[e], key[e], wvv, wk) && bm_better(v[e], key[e], bv, bk)) { bv = v[e]; bk = key[e]; }
    }
  }
  __syncthreads();
  return cnt;
}

template <bool VEC>
__global__ __launch_bounds__(BM_T) void beam_slice_kernel(BeamP a) {
  __shared__ __attribute__((aligned(16))) unsigned char map[BM_SLICE];  // 0, 1: penalised, 2: banned
  __shared__ float red_v[2][BM_W], out_v[BM_KMAX];
  __shared__ int red_k[2][BM_W], out_k[BM_KMAX];
  const int r = blockIdx.x / BM_G, g = blockIdx.x % BM_G, tid = threadIdx.x;
  const int n = a.n, b = r / n, j = r - b * n;
  if (a.done[b] != 0) return;  // (uniform)
  if (a.live[r] == 0) {        // a dead beam contributes no candidates
    if (tid == 0) a.cand_n[(long)r * BM_G + g] = 0;
    return;
  }
  const int V = a.V, K = 2 * n;
  const float* x = a.logits + (long)r * V;
  int lo4, hi4;
  bm_slice(V, g, lo4, hi4);
  const long lo = 4L * lo4, hi = min(4L * hi4, (long)V);
  // ---- which of the slice's tokens the history penalises or bans (HF: RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor)
  reinterpret_cast<u32x4*>(map)[tid] = u32x4{0u, 0u, 0u, 0u};  // BM_SLICE = 16 * BM_T bytes
  __syncthreads();
  const long* hist = a.history + (long)r * a.hist_cap;
  const int hl = min(max(a.hist_len[r], 0), a.hist_cap);
  if (a.penalty != 1.f) {
    for (int i = tid; i < hl; i += BM_T) {
      const long t = hist[i];
      if (t >= lo && t < hi) map[t - lo] = 1;  // (every writer of a byte writes the same value)
    }
    __syncthreads();
  }
  const int ng = a.ngram;
  if (ng > 0 && hl + 1 >= ng) {
    for (int i = tid; i + ng - 1 < hl; i += BM_T) {
      bool match = true;
      for (int k = 0; k < ng - 1 && match; ++k) match = hist[i + k] == hist[hl - (ng - 1) + k];
      const long t = hist[i + ng - 1];
      if (match && t >= lo && t < hi) map[t - lo] = 2;
    }
    __syncthreads();
  }
  // ---- the row's (M, log S): the 16 partials in slice order, as logprob_finish adds them
  const float* pm = a.part_m + (long)r * BM_G;
  const float* ps = a.part_s + (long)r * BM_G;
  float M = pm[0];
#pragma unroll
  for (int q = 1; q < BM_G; ++q) M = fmaxf(M, pm[q]);
  float S = 0.f;
#pragma unroll
  for (int q = 0; q < BM_G; ++q) S += ps[q] * expf(pm[q] - M);
  const float logS = logf(S);
  const float run = a.run_score[r], pen = a.penalty;
  // ---- the slice's processed scores, in registers
  float v[4 * BM_E4];
  int key[4 * BM_E4];
#pragma unroll
  for (int e = 0; e < BM_E4; ++e) {
    const int i4 = lo4 + tid + e * BM_T;
    const f32x4 t = bm_load4<VEC>(x, i4, hi4, V);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long idx = 4L * i4 + c;
      float s_ = -INFINITY;
      int k_ = BM_NOKEY;
      if (i4 < hi4 && idx < V) {
        float lp = (t[c] - M) - logS;
        const unsigned char f = map[idx - lo];
        if (f == 1) lp = lp < 0.f ? lp * pen : lp / pen;
        if (f == 2) lp = -INFINITY;
        s_ = lp + run;
        k_ = j * V + (int)idx;
      }
      v[4 * e + c] = s_;
      key[4 * e + c] = k_;
    }
  }
  const int cnt = bm_block_topk<4 * BM_E4>(v, key, K, out_v, out_k, red_v, red_k);
  const long slot0 = ((long)r * BM_G + g) * BM_KMAX;
  if (tid < cnt) {
    a.cand_v[slot0 + tid] = out_v[tid];
    a.cand_k[slot0 + tid] = out_k[tid];
  }
  if (tid == 0) a.cand_n[(long)r * BM_G + g] = cnt;
}

constexpr int BM_ME = BM_NMAX * BM_G * BM_KMAX / BM_T;  // slice candidates per thread of the merge: 8
constexpr int BM_FROM_CAND = 64;                        // finished-store source codes: old slot o, or BM_FROM_CAND + candidate k

__global__ __launch_bounds__(BM_T) void beam_merge_kernel(BeamP a) {
  __shared__ float red_v[2][BM_W], cv[BM_KMAX];
  __shared__ int red_k[2][BM_W], ck[BM_KMAX];
  __shared__ int new_par[BM_NMAX], new_live[BM_NMAX], src[BM_NMAX], slot_len[BM_NMAX], s_done, s_moved;
  __shared__ long new_tok[BM_NMAX];
  __shared__ float new_score[BM_NMAX], slot_score[BM_NMAX], ms[BM_KMAX];
  __shared__ int mf[BM_KMAX], ml[BM_KMAX], stop[BM_KMAX];  // (thread 0's lists: LDS, so that no thread needs scratch)
  const int b = blockIdx.x, tid = threadIdx.x, n = a.n, V = a.V, N = a.N, K = 2 * n;
  const long r0 = (long)b * n;
  const int s = a.step[b];
  if (a.done[b] != 0 || s < 0 || s >= N) {  // (uniform) inert: the rows keep their state, the reorder skips the prompt
    if (tid < n) a.parent[r0 + tid] = tid;
    if (tid == 0) a.plan[4 * b] = -1;
    return;
  }
  // ---- the K best of the n * 16 slice lists
  float v[BM_ME];
  int key[BM_ME];
#pragma unroll
  for (int e = 0; e < BM_ME; ++e) {
    const int q = tid + e * BM_T, j = q / (BM_G * BM_KMAX), rem = q % (BM_G * BM_KMAX), g = rem / BM_KMAX, k = rem % BM_KMAX;
    v[e] = -INFINITY;
    key[e] = BM_NOKEY;
    if (j < n) {
      const long rg = (r0 + j) * BM_G + g;
      if (k < min(a.cand_n[rg], BM_KMAX)) {
        v[e] = a.cand_v[rg * BM_KMAX + k];
        key[e] = a.cand_k[rg * BM_KMAX + k];
      }
    }
  }
  const int cnt = bm_block_topk<BM_ME>(v, key, K, cv, ck, red_v, red_k);
  const bool last = s + 1 == N;
  const float lpow = a.len_pow[s];
  const int gen_cap = a.hist_cap;
  if (tid == 0) {
    bool all_stop = cnt > 0;
    for (int k = 0; k < cnt; ++k) {
      stop[k] = last || (a.eos >= 0 && (long)(ck[k] % V) == a.eos);
      all_stop = all_stop && stop[k] != 0;
    }
    // new running beams: the first n candidates that do not stop
    int m = 0;
    for (int k = 0; k < cnt && m < n; ++k)
      if (!stop[k]) {
        new_par[m] = ck[k] / V;
        new_tok[m] = ck[k] % V;
        new_score[m] = cv[k];
        new_live[m] = 1;
        ++m;
      }
    const int n_live = m;
    for (; m < n; ++m) { new_par[m] = m; new_tok[m] = a.pad; new_score[m] = -INFINITY; new_live[m] = 0; }
    // finished store: the old slots, then the admitted candidates in candidate order; the n best, stable
    const bool old_unsat = a.unsat[b] != 0;
    bool all_flag = true;
    for (int i = 0; i < n; ++i) all_flag = all_flag && a.fin_flag[r0 + i] != 0;
    const bool admit = old_unsat && !(all_flag && a.early != 0);
    int nm = 0;
    auto insert = [&](float sc, int from, int len) {
      int p = nm;
      while (p > 0 && sc > ms[p - 1]) { ms[p] = ms[p - 1]; mf[p] = mf[p - 1]; ml[p] = ml[p - 1]; --p; }
      ms[p] = sc; mf[p] = from; ml[p] = len;
      ++nm;
    };
    for (int i = 0; i < n; ++i)
      if (a.fin_flag[r0 + i] != 0) insert(a.fin_score[r0 + i], i, a.fin_len[r0 + i]);
    for (int k = 0; k < cnt && k < n; ++k)
      if (stop[k] && admit) insert(cv[k] / lpow, BM_FROM_CAND + k, s + 1);
    const int n_fin = min(nm, n);
    float worst = INFINITY;
    for (int i = 0; i < n; ++i) {
      src[i] = i < n_fin ? mf[i] : -1;
      slot_score[i] = i < n_fin ? ms[i] : 0.f;
      slot_len[i] = i < n_fin ? ml[i] : 0;
      if (i < n_fin) worst = fminf(worst, ms[i]);
    }
    // early-stop heuristic, then whether the prompt is done
    const bool improve = n_fin < n || (n_live > 0 && new_score[0] / lpow > worst);
    const bool unsat = old_unsat && improve;
    s_done = !unsat || (n_fin == n && a.early != 0) || all_stop;
    bool moved = false;
    for (int i = 0; i < n; ++i) moved = moved || new_par[i] != i;
    s_moved = moved;
    a.unsat[b] = unsat;
  }
  __syncthreads();
  // ---- the finished store, in place: an old slot only ever moves down, so the slots are filled from the last one up
  long* ft = a.fin_tokens + r0 * N;
  for (int i = n - 1; i >= 0; --i) {
    const int o = src[i];
    if (o >= 0 && o < BM_FROM_CAND && o != i)
      for (int t = tid; t < N; t += BM_T) ft[(long)i * N + t] = ft[(long)o * N + t];
    __syncthreads();
  }
  for (int i = 0; i < n; ++i) {
    const int o = src[i];
    if (o >= BM_FROM_CAND) {  // candidate k: its parent's generated tokens, the token, pad behind
      const int k = o - BM_FROM_CAND, par = ck[k] / V;
      const long rp = r0 + par;
      const int gen0 = max(min(max(a.hist_len[rp], 0), gen_cap) - s, 0);
      const long* h = a.history + rp * a.hist_cap + gen0;
      for (int t = tid; t < N; t += BM_T) ft[(long)i * N + t] = t < s ? h[t] : (t == s ? (long)(ck[k] % V) : a.pad);
    }
  }
  if (tid < n) {
    const long r = r0 + tid;
    a.fin_score[r] = slot_score[tid];
    a.fin_flag[r] = src[tid] >= 0;
    a.fin_len[r] = slot_len[tid];
    a.parent[r] = new_par[tid];
    a.cur_tok[r] = new_tok[tid];
    a.run_score[r] = new_score[tid];
    a.live[r] = new_live[tid];
    a.finished[r] = s_done;
  }
  if (tid == 0) {
    a.done[b] = s_done;
    a.plan[4 * b + 0] = s;
    a.plan[4 * b + 1] = s > 0 ? max(a.pos[r0] - a.prefix_len[b] + 1, 0) : 0;  // suffix slots written so far
    a.plan[4 * b + 2] = s_moved;
    a.plan[4 * b + 3] = max(min(max(a.hist_len[r0], 0), gen_cap) - s, 0);  // where the generated part of a history starts
  }
  if (a.trace && tid < K) {
    int* t = a.trace + (((long)s * (a.R / n) + b) * K + tid) * 3;
    t[0] = tid < cnt ? ck[tid] / V : -1;
    t[1] = tid < cnt ? ck[tid] % V : -1;
    t[2] = tid < cnt ? __float_as_int(cv[tid]) : 0;
  }
}

// ---------------------------------------------------------------------------
// tcavt_beam_reorder
// ---------------------------------------------------------------------------
struct ReorderP {
  const int* parent;
  const int* plan;
  const long* cur_tok;
  long* history;
  int* hist_len;
  int* pos;
  int* step;
  unsigned char* kv[2];
  long n_copy;  // 2 * n_layers * B * suffix_lmax * ppr
  int B, n, hist_cap, n_layers, suffix_lmax, ppr;  // ppr: 16-byte pieces of a cache row (nkv * 8)
};

// regs[p] with a uniform p, without indexing the register array by a variable
template <class T, int J = 0>
__device__ __forceinline__ T bm_pick(const T (&regs)[BM_NMAX], int p) {
  if constexpr (J == BM_NMAX - 1) {
    return regs[J];
  } else {
    if (p == J) return regs[J];
    return bm_pick<T, J + 1>(regs, p);
  }
}

// The n rows of one position, in place: everything that is somebody's parent is loaded before anything is stored.
// at(j): the address of row j's element; par[j] in [0, n).
template <class T, class At>
__device__ __forceinline__ void bm_permute(int n, const int (&par)[BM_NMAX], At at) {
  unsigned int need = 0;
#pragma unroll
  for (int j = 0; j < BM_NMAX; ++j)
    if (j < n && par[j] != j) need |= 1u << par[j];
  T regs[BM_NMAX];
#pragma unroll
  for (int j = 0; j < BM_NMAX; ++j)
    if (j < n && ((need >> j) & 1u)) regs[j] = *at(j);
#pragma unroll
  for (int j = 0; j < BM_NMAX; ++j)
    if (j < n && par[j] != j) *at(j) = bm_pick<T>(regs, par[j]);
}

__device__ __forceinline__ void bm_parents(const ReorderP& a, int b, int (&par)[BM_NMAX]) {
#pragma unroll
  for (int j = 0; j < BM_NMAX; ++j) {
    par[j] = j;
    if (j < a.n) {
      const int p = a.parent[(long)b * a.n + j];
      if (p >= 0 && p < a.n) par[j] = p;
    }
  }
}

__global__ __launch_bounds__(256) void beam_reorder_kernel(ReorderP a) {
  const long first_state = (long)gridDim.x - a.B;
  const int n = a.n;
  if (blockIdx.x >= first_state) {
    // ---- the histories of prompt b: the generated part follows the parents, then the new token
    const int b = (int)(blockIdx.x - first_state);
    const int s = a.plan[4 * b];
    if (s < 0) return;  // (uniform) done before this step
    const long r0 = (long)b * n;
    if (a.plan[4 * b + 2] != 0) {
      int par[BM_NMAX];
      bm_parents(a, b, par);
      const int gen0 = a.plan[4 * b + 3];
      for (int i = threadIdx.x; i < s && gen0 + i < a.hist_cap; i += 256)
        bm_permute<long>(n, par, [&](int j) { return a.history + (r0 + j) * a.hist_cap + gen0 + i; });
    }
    __syncthreads();
    if ((int)threadIdx.x < n) {
      const long r = r0 + threadIdx.x;
      const int hl = a.hist_len[r];
      if (hl >= 0 && hl < a.hist_cap) {
        a.history[r * a.hist_cap + hl] = a.cur_tok[r];
        a.hist_len[r] = hl + 1;
      }
      if (s > 0) a.pos[r] += 1;
    }
    if (threadIdx.x == 0) a.step[b] = s + 1;
    return;
  }
  // ---- one 16-byte piece position of the suffix caches
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_copy) return;
  const int piece = (int)(i % a.ppr);
  long q = i / a.ppr;
  const int slot = (int)(q % a.suffix_lmax);
  q /= a.suffix_lmax;
  const int b = (int)(q % a.B);
  q /= a.B;
  const int layer = (int)(q % a.n_layers), kv = (int)(q / a.n_layers);
  if (a.plan[4 * b] < 0 || a.plan[4 * b + 2] == 0 || slot >= min(a.plan[4 * b + 1], a.suffix_lmax)) return;
  int par[BM_NMAX];
  bm_parents(a, b, par);
  u32x4* base = reinterpret_cast<u32x4*>(a.kv[kv]);
  const long R = (long)a.B * n;
  bm_permute<u32x4>(n, par, [&](int j) {
    return base + (((long)layer * R + (long)b * n + j) * a.suffix_lmax + slot) * a.ppr + piece;
  });
}

static inline int64_t bm_align(int64_t x) { return (x + 15) & ~(int64_t)15; }

}  // namespace tcavt

using namespace tcavt;

extern "C" int64_t tcavt_beam_workspace_bytes(int R) {
  if (R <= 0) return 0;
  const int64_t r = R;
  return 2 * bm_align(r * BM_G * 4) + bm_align(r * BM_G * 4) + 2 * bm_align(r * BM_G * BM_KMAX * 4);
}

extern "C" int tcavt_beam_select(const tcavt_beam_args* a, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(a, "beam_select: args is a null pointer");
  const struct { const void* p; const char* name; } ptrs[] = {
      {a->logits, "logits"}, {a->history, "history"}, {a->hist_len, "hist_len"}, {a->run_score, "run_score"}, {a->live, "live"},
      {a->fin_tokens, "fin_tokens"}, {a->fin_score, "fin_score"}, {a->fin_flag, "fin_flag"}, {a->fin_len, "fin_len"},
      {a->unsat, "unsat"}, {a->done, "done"}, {a->cur_tok, "cur_tok"}, {a->pos, "pos"}, {a->finished, "finished"}, {a->step, "step"},
      {a->prefix_len, "prefix_len"}, {a->len_pow, "len_pow"}, {a->parent, "parent"}, {a->plan, "plan"}, {a->workspace, "workspace"}};
  for (const auto& q : ptrs) TCAVT_CHECK_ARG(q.p, "beam_select: %s is a null pointer", q.name);
  TCAVT_CHECK_ARG(a->n >= 2 && a->n <= BM_NMAX, "beam_select: n = %d must be in [2, %d]", a->n, BM_NMAX);
  TCAVT_CHECK_ARG(a->R > 0 && a->R % a->n == 0, "beam_select: R = %d must be a positive multiple of n = %d", a->R, a->n);
  TCAVT_CHECK_ARG(a->V >= 2 * a->n, "beam_select: V = %d must be >= 2 n = %d", a->V, 2 * a->n);
  TCAVT_CHECK_ARG(a->V <= BM_VMAX, "beam_select: V = %d must be <= %d", a->V, BM_VMAX);
  TCAVT_CHECK_ARG(a->N >= 1, "beam_select: N = %d must be >= 1", a->N);
  TCAVT_CHECK_ARG(a->hist_cap > 0, "beam_select: hist_cap = %d must be > 0", a->hist_cap);
  TCAVT_CHECK_ARG(a->no_repeat_ngram_size >= 0, "beam_select: no_repeat_ngram_size = %d must be >= 0", a->no_repeat_ngram_size);
  TCAVT_CHECK_ARG(a->repetition_penalty > 0.f, "beam_select: repetition_penalty must be > 0");
  const int64_t need = tcavt_beam_workspace_bytes(a->R);
  TCAVT_CHECK_ARG(a->workspace_bytes >= need, "beam_select: workspace_bytes = %lld, needs %lld", (long long)a->workspace_bytes, (long long)need);
  TCAVT_CHECK_ARG(aligned16(a->workspace), "beam_select: workspace must be 16-byte aligned");
  BeamP p;
  p.logits = a->logits; p.history = reinterpret_cast<const long*>(a->history); p.hist_len = a->hist_len;
  p.run_score = a->run_score; p.live = a->live; p.fin_tokens = reinterpret_cast<long*>(a->fin_tokens); p.fin_score = a->fin_score;
  p.fin_flag = a->fin_flag; p.fin_len = a->fin_len; p.unsat = a->unsat; p.done = a->done;
  p.cur_tok = reinterpret_cast<long*>(a->cur_tok); p.pos = a->pos; p.finished = a->finished; p.step = a->step;
  p.prefix_len = a->prefix_len; p.len_pow = a->len_pow; p.parent = a->parent; p.plan = a->plan; p.trace = a->trace;
  char* w = static_cast<char*>(a->workspace);
  const int64_t R = a->R;
  p.part_m = reinterpret_cast<float*>(w); w += bm_align(R * BM_G * 4);
  p.part_s = reinterpret_cast<float*>(w); w += bm_align(R * BM_G * 4);
  p.cand_n = reinterpret_cast<int*>(w); w += bm_align(R * BM_G * 4);
  p.cand_v = reinterpret_cast<float*>(w); w += bm_align(R * BM_G * BM_KMAX * 4);
  p.cand_k = reinterpret_cast<int*>(w);
  p.eos = a->eos_token_id; p.pad = a->pad_token_id; p.penalty = a->repetition_penalty; p.ngram = a->no_repeat_ngram_size;
  p.early = a->early_stopping; p.R = a->R; p.n = a->n; p.V = a->V; p.N = a->N; p.hist_cap = a->hist_cap;
  const bool vec = (p.V & 3) == 0 && aligned16(p.logits);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vec ? beam_partial_kernel<true> : beam_partial_kernel<false>, dim3(p.R * BM_G), dim3(BM_T), 0, st, p);
  hipLaunchKernelGGL(vec ? beam_slice_kernel<true> : beam_slice_kernel<false>, dim3(p.R * BM_G), dim3(BM_T), 0, st, p);
  hipLaunchKernelGGL(beam_merge_kernel, dim3(p.R / p.n), dim3(BM_T), 0, st, p);
  TCAVT_CHECK_LAUNCH("beam_select");
  return TCAVT_OK;
}

extern "C" int tcavt_beam_reorder(const tcavt_beam_reorder_args* a, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(a, "beam_reorder: args is a null pointer");
  const struct { const void* p; const char* name; } ptrs[] = {
      {a->parent, "parent"}, {a->plan, "plan"}, {a->cur_tok, "cur_tok"}, {a->history, "history"}, {a->hist_len, "hist_len"},
      {a->pos, "pos"}, {a->step, "step"}, {a->suffix_k, "suffix_k"}, {a->suffix_v, "suffix_v"}};
  for (const auto& q : ptrs) TCAVT_CHECK_ARG(q.p, "beam_reorder: %s is a null pointer", q.name);
  TCAVT_CHECK_ARG(a->n >= 2 && a->n <= BM_NMAX, "beam_reorder: n = %d must be in [2, %d]", a->n, BM_NMAX);
  TCAVT_CHECK_ARG(a->R > 0 && a->R % a->n == 0, "beam_reorder: R = %d must be a positive multiple of n = %d", a->R, a->n);
  TCAVT_CHECK_ARG(a->hist_cap > 0, "beam_reorder: hist_cap = %d must be > 0", a->hist_cap);
  TCAVT_CHECK_ARG(a->n_layers > 0 && a->nkv > 0 && a->suffix_lmax > 0, "beam_reorder: bad shape (n_layers, nkv, suffix_lmax > 0)");
  TCAVT_CHECK_ARG(aligned16(a->suffix_k) && aligned16(a->suffix_v), "beam_reorder: the suffix caches must be 16-byte aligned");
  ReorderP p;
  p.parent = a->parent; p.plan = a->plan; p.cur_tok = reinterpret_cast<const long*>(a->cur_tok);
  p.history = reinterpret_cast<long*>(a->history); p.hist_len = a->hist_len; p.pos = a->pos; p.step = a->step;
  p.kv[0] = static_cast<unsigned char*>(a->suffix_k); p.kv[1] = static_cast<unsigned char*>(a->suffix_v);
  p.B = a->R / a->n; p.n = a->n; p.hist_cap = a->hist_cap; p.n_layers = a->n_layers; p.suffix_lmax = a->suffix_lmax;
  p.ppr = a->nkv * 8;
  p.n_copy = 2L * a->n_layers * p.B * a->suffix_lmax * p.ppr;
  const long blocks = (p.n_copy + 255) / 256 + p.B;
  TCAVT_CHECK_ARG(blocks <= 0x7fffffffL, "beam_reorder: too many rows");
  hipLaunchKernelGGL(beam_reorder_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  TCAVT_CHECK_LAUNCH("beam_reorder");
  return TCAVT_OK;
}
