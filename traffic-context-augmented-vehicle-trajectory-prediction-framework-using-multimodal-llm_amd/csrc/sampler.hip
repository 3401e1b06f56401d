// Token selection of text generation (include/tcavt.h: tcavt_sample_logits, tcavt_sample_logits_slots, tcavt_sample_logits_rows,
// tcavt_sample_tokens, tcavt_sample_tokens_per_request, tcavt_request_params_check, tcavt_sample_workspace_bytes): the logits
// processors, the ending rules and the draw -- the parameters by value or, per request, from a device table --, the last launches of a
// decode step (csrc/generate.hip).  They also advance the per-row state (history, position, step, finished) on the device.
#include "common.hpp"
#include "philox.hpp"

namespace tcavt {

// ---------------------------------------------------------------------------
// Logits processors + token selection, one workgroup per sample (HF generation: RepetitionPenaltyLogitsProcessor,
// NoRepeatNGramLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper, in that order; the warpers
// only when sampling).  `logits` is modified in place (penalty / bans).  The candidates that survive top-k are gathered
// in descending (value, then ascending index) order by k rounds of a block-wide arg-max "next after the previous one" --
// exact ties at the k-th value are all kept, as `scores < topk[-1]` keeps them.
// ---------------------------------------------------------------------------
struct SampleP {
  float temperature, top_p, rep_penalty;
  int top_k, no_repeat_ngram, do_sample;
  long eos, pad;
  unsigned int seed_lo, seed_hi;
};

// Ending rules of a request (tcavt_stop_rules; sample kernels with STOP): a stop set as a bitmap over the vocabulary, up to
// SMP_SEQS stop sequences of 1 .. SMP_SEQ_LEN ids, the ban of every ending token while step < min_new
// (MinNewTokensLengthLogitsProcessor with eos_token_id given as a list), and the record of how and when a request ended.
struct StopP {
  const unsigned int* bitmap;  // [(V + 31) / 32], bit id & 31 of word id >> 5; or NULL
  const long* seqs;            // [n_seqs][SMP_SEQ_LEN]
  const int* seq_len;          // [n_seqs]; a length outside [1, SMP_SEQ_LEN] never matches
  int* finish_reason;          // indexed like out_tokens' rows; or NULL
  int* n_generated;            // likewise
  int n_seqs, min_new;
};
constexpr int SMP_SEQS = 16, SMP_SEQ_LEN = 8;

// Per-request parameters (tcavt_request_params; sample kernels with REQ): the workgroup of a row reads its SampleP and its own
// min_new from device tables at the row's request index r -- the row b in the batch form, out_row[sb] in the slots and rows forms --
// in the place of the kernel arguments, and runs the same code on them: r, and with it every branch on the parameters, is uniform
// per workgroup.  pad stays the call's.  A row whose r lies outside [0, n_req) reads nothing of the table, writes nothing and sets
// bit 0 of *bad_flag.
struct ReqP {
  const tcavt_sample_params* table;  // [n_req]
  const int* min_new;                // [n_req]; or NULL: StopP.min_new
  int* bad_flag;                     // or NULL
  const long* out_row;               // slots and rows forms (the kernels' out_row); NULL in the batch form
  long pad;
  int n_req;
};
template <bool REQ> struct sample_arg { typedef SampleP type; };
template <> struct sample_arg<true> { typedef ReqP type; };
// (without REQ `sp` names the kernel argument itself: those instantiations are the code they were before REQ existed)
__device__ __forceinline__ const SampleP& params_of(const SampleP& arg, const SampleP&) { return arg; }
__device__ __forceinline__ const SampleP& params_of(const ReqP&, const SampleP& fetched) { return fetched; }
__device__ __forceinline__ SampleP request_params(const ReqP& rq, long r) {
  const tcavt_sample_params* __restrict__ t = rq.table + r;
  SampleP p;
  p.temperature = t->temperature; p.top_p = t->top_p; p.rep_penalty = t->repetition_penalty;
  p.top_k = t->top_k; p.no_repeat_ngram = t->no_repeat_ngram_size; p.do_sample = t->do_sample;
  p.eos = t->eos_token_id; p.pad = rq.pad;
  const unsigned long seed = t->seed;
  p.seed_lo = (unsigned int)(seed & 0xffffffffu); p.seed_hi = (unsigned int)(seed >> 32);
  return p;
}
constexpr int FIN_EOS = 1, FIN_STOP_TOKEN = 2, FIN_STOP_SEQ = 3, FIN_BUDGET = 4;

constexpr int SMP_T = 1024;   // threads
constexpr int SMP_CAP = 256;  // candidate list capacity (top_k + ties)
constexpr int SMP_BINS = 2048;  // histogram of (max - score) * 64: covers 32 units below the maximum
constexpr int SMP_LIST = 1024;  // pre-selected scores (everything down to the threshold bin)
static_assert(SMP_LIST <= SMP_T && (SMP_BINS / 64 & (SMP_BINS / 64 - 1)) == 0, "one thread per list entry; bins per lane a power of two");

__device__ __forceinline__ bool after(float v, int i, float pv, int pi) {  // (v, i) comes after (pv, pi) in (value desc, index asc) order
  return v < pv || (v == pv && i > pi);
}
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) {  // (v, i) precedes (bv, bi)
  return v > bv || (v == bv && i < bi);
}

// ---------------------------------------------------------------------------
// Two-stage form (round 4; tcavt_sample_logits with a workspace): one workgroup per sample walks 128 256 logits in three
// dependent passes -- 64 us on 8 of 256 CUs at B = 8, latency bound.  Stage 1 cuts every sample's vocabulary into SMP_G
// contiguous slices, one workgroup each (B x 16 workgroups): the slice's processors (a token's penalty / ban is applied by the
// workgroup that owns the token), then the slice's <= 8 scores per thread live in REGISTERS and the three passes (max / min,
// histogram, collection) cost no further memory traffic; out come the slice's candidates -- everything at or above the slice's
// own top-k threshold bin -- and the smallest of them, lb: at least k scores of the slice are >= lb, so the sample's k-th
// largest score is >= lb too.  Stage 2 (sample_kernel with `pre`) keeps the candidates >= max over the slices of lb (a superset
// of the global top-k and of every tie with the k-th value), and ranks / keeps / draws exactly as the one-stage form does:
// the selected token is the same.  A slice whose threshold bin overflows its list (e.g. constant logits) raises ovf[b] and the
// sample falls back to the three passes of the one-stage form (its processors are done).
// ---------------------------------------------------------------------------
// Does token t occur among the first n entries of an LDS-resident history?  Four entries per LDS read and NO early exit: written
// as "scan until found", thread i's loop is a chain of up to i dependent LDS round trips (one ~100-cycle latency per entry:
// 15 us for a 300-token history -- a quarter of the whole selection kernel); without the data-dependent exit the reads pipeline.
__device__ __forceinline__ bool occurs_before(const int* __restrict__ lds_tok, int n, int t) {
  typedef __attribute__((ext_vector_type(4))) int i32x4;
  bool dup = false;
  int j = 0;
#pragma unroll 4
  for (; j + 4 <= n; j += 4) {
    const i32x4 q = *reinterpret_cast<const i32x4*>(lds_tok + j);
    dup |= (q[0] == t) | (q[1] == t) | (q[2] == t) | (q[3] == t);
  }
  for (; j < n; ++j) dup |= lds_tok[j] == t;
  return dup;
}

constexpr int SMP_G = 16;      // slices (stage-1 workgroups) per sample
constexpr int SMP_LCAP = 512;  // candidates per slice
constexpr int SMP_E4 = 4;      // f32x4 registers per thread: slices of up to 4 * 1024 * 4 scores (V <= 262 144)

struct SliceWs {  // views into the caller's workspace (tcavt_sample_logits: layout and size)
  int* ticket;    // [1]   stage 2: workgroups that have read *step (the last one increments it); zero between calls
  int* ovf;       // [B]   a slice of the sample overflowed its list; zero between calls
  int* cand_n;    // [B][G]
  float* lb;      // [B][G]
  float* cand_v;  // [B][G][SMP_LCAP]
  int* cand_i;    // [B][G][SMP_LCAP]
};

// STOP: the ban of the ending tokens before the minimum (StopP) -- the workgroup that owns a token bans it, as with the other
// processors: the four ids of a lane's f32x4 lie in one word of the bitmap, so one load serves all four, and the banned scores go
// back to the row (the one-stage fallback of stage 2 reads them there).  The branch is uniform per row and nothing is loaded for
// the ban once the minimum is reached.  step_p: the row's step word (per_slot: step_p[sb], else *step_p).
// REQ: the parameters come from the request tables (ReqP).
template <bool STOP = false, bool REQ = false>
__global__ __launch_bounds__(SMP_T) void sample_slice_kernel(float* __restrict__ logits, int V, const long* __restrict__ history,
                                                             int hist_cap, const int* __restrict__ hist_len,
                                                             typename sample_arg<REQ>::type spa, SliceWs ws,
                                                             const int* __restrict__ slot_of_row, int S, StopP sr,
                                                             const int* __restrict__ step_p, int per_slot,
                                                             const int* __restrict__ finished) {
  __shared__ int hist_bins[SMP_BINS];
  __shared__ float lv[SMP_LCAP];
  __shared__ __attribute__((aligned(16))) int li[SMP_LCAP];
  __shared__ float rv[SMP_T / 64], rm[SMP_T / 64];
  __shared__ int ri[SMP_T / 64];
  __shared__ float s_max, s_min;
  __shared__ int s_bi, list_n, thr_bin;
  const int b = blockIdx.x / SMP_G, g = blockIdx.x % SMP_G, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // (slot_of_row: logits row b belongs to slot sb of the state arrays; a row without a slot is skipped, nothing of it is written)
  const int sb = slot_of_row ? slot_of_row[b] : b;
  if (sb < 0 || sb >= S) return;  // (uniform)
  [[maybe_unused]] SampleP sp_req;
  const SampleP& sp = params_of(spa, sp_req);
  [[maybe_unused]] const int* req_min = nullptr;  // REQ: the request's own minimum, when the call has them
  if constexpr (REQ) {
    const long r = spa.out_row ? spa.out_row[sb] : (long)b;
    if (r < 0 || r >= (long)spa.n_req) return;  // (uniform) inert; stage 2 raises the flag
    sp_req = request_params(spa, r);
    if (spa.min_new) req_min = spa.min_new + r;
  }
  float* x = logits + (long)b * V;
  const long* hist = history + (long)sb * hist_cap;
  const int hl = min(hist_len[sb], hist_cap);
  const int V4 = V >> 2, chunk4 = (V4 + SMP_G - 1) / SMP_G;
  const int lo4 = g * chunk4, hi4 = min(lo4 + chunk4, V4);
  const long lo = 4L * lo4, hi = 4L * hi4;
  // ---- processors, for the tokens this slice owns (same arithmetic and order as the one-stage form: penalty, then ban)
  // (the history goes to LDS once when it fits, and both processors read it there: every global access the processors make is
  //  one more dependent round trip at the head of a kernel that is a handful of them long)
  const bool in_lds = hl <= SMP_LCAP;
  const int ng = sp.no_repeat_ngram;
  const bool do_rep = sp.rep_penalty != 1.f, do_ban = ng > 0 && hl + 1 >= ng;
  if (in_lds && (do_rep || do_ban)) {
    for (int i = tid; i < hl; i += SMP_T) li[i] = (int)min(max(hist[i], -1L), 0x7fffffffL);  // (ids >= 2^31 - 1 are out of range anyway)
    __syncthreads();
  }
  auto tok_at = [&](int i) -> long { return in_lds ? (long)li[i] : hist[i]; };
  if (do_rep) {
    for (int i = tid; i < hl; i += SMP_T) {
      const long t = tok_at(i);
      bool first = t >= lo && t < hi;
      if (in_lds) {
        first = first && !occurs_before(li, i, (int)t);
      } else {
        for (int j = 0; j < i && first; ++j) first = hist[j] != t;
      }
      if (first) {
        const float s_ = x[t];
        x[t] = s_ < 0.f ? s_ * sp.rep_penalty : s_ / sp.rep_penalty;
      }
    }
    __syncthreads();
  }
  if (do_ban) {
    for (int i = tid; i + ng - 1 < hl; i += SMP_T) {
      bool match = true;
      for (int k = 0; k < ng - 1 && match; ++k) {
        const int p = i + k, q = hl - (ng - 1) + k;
        const long a = tok_at(p);
        match = a == tok_at(q);
        // (the LDS copy folds every id below 0 onto -1 and every id from 2^31 - 1 up onto 2^31 - 1: two of those are equal only
        //  if the ids themselves are, as in the one-stage form)
        if (match && in_lds && (a == -1L || a == 0x7fffffffL)) match = hist[p] == hist[q];
      }
      const long t = tok_at(i + ng - 1);
      if (match && t >= lo && t < hi) x[t] = -INFINITY;
    }
    __syncthreads();
  }
  // ---- the slice, in registers (scaled by 1 / temperature when sampling: the order of the scores is what counts)
  const float sc = sp.do_sample ? 1.f / sp.temperature : 1.f;
  f32x4 v4[SMP_E4];
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
  bool min_ban = false;  // (uniform)
  if constexpr (STOP) {
    int min_new = sr.min_new;
    if constexpr (REQ) {
      if (req_min) min_new = *req_min;
    }
    if (min_new > 0) min_ban = (per_slot ? step_p[sb] : *step_p) < min_new && finished[sb] == 0;
  }
#pragma unroll
  for (int e = 0; e < SMP_E4; ++e) {
    const int i4 = lo4 + tid + e * SMP_T;
    f32x4 t = i4 < hi4 ? x4[i4] : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};  // (a padding -inf never precedes a real entry: its index is larger)
    if constexpr (STOP) {
      if (min_ban && i4 < hi4) {
        unsigned int m = sr.bitmap ? (sr.bitmap[i4 >> 3] >> ((i4 & 7) * 4)) & 15u : 0u;
        if (sp.eos >= 0 && (sp.eos >> 2) == (long)i4) m |= 1u << (int)(sp.eos & 3);
        if (m) {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if ((m >> c) & 1u) t[c] = -INFINITY;
          reinterpret_cast<f32x4*>(x)[i4] = t;
        }
      }
    }
    v4[e] = t * sc;
  }
  // best (value desc, index asc) and smallest finite score of the slice
  float bv = -INFINITY, lmin = INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int e = 0; e < SMP_E4; ++e) {
    const int i4 = lo4 + tid + e * SMP_T;
    if (i4 < hi4) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float v = v4[e][c];
        const int i = 4 * i4 + c;
        if (better(v, i, bv, bi)) { bv = v; bi = i; }
        if (v > -INFINITY) lmin = fminf(lmin, v);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  lmin = -wave_max(-lmin);
  if (lane == 0) { rv[wv] = bv; ri[wv] = bi; rm[wv] = lmin; }
  __syncthreads();
  if (tid == 0) {
    float v = rv[0], m_ = rm[0];
    int i = ri[0];
    for (int k = 1; k < SMP_T / 64; ++k) {
      if (better(rv[k], ri[k], v, i)) { v = rv[k]; i = ri[k]; }
      m_ = fminf(m_, rm[k]);
    }
    s_max = v; s_bi = i; s_min = m_;
    list_n = 0;
  }
  for (int i = tid; i < SMP_BINS; i += SMP_T) hist_bins[i] = 0;
  __syncthreads();
  const long slot0 = ((long)b * SMP_G + g) * SMP_LCAP;
  if (!sp.do_sample) {  // greedy: the slice's first maximum
    if (tid == 0) {
      ws.cand_v[slot0] = s_max;
      ws.cand_i[slot0] = s_bi;
      ws.cand_n[b * SMP_G + g] = 1;
      ws.lb[b * SMP_G + g] = -INFINITY;
    }
    return;
  }
  const float gmax = s_max;
  if (!(gmax > -INFINITY)) {  // (uniform) nothing finite in this slice
    if (tid == 0) { ws.cand_n[b * SMP_G + g] = 0; ws.lb[b * SMP_G + g] = -INFINITY; }
    return;
  }
  const float bscale = (float)(SMP_BINS - 1) / fmaxf(gmax - s_min, 1e-20f);
  const int k = min(max(sp.top_k, 1), SMP_CAP);
#pragma unroll
  for (int e = 0; e < SMP_E4; ++e) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float d = (gmax - v4[e][c]) * bscale;
      if (d < (float)SMP_BINS) atomicAdd(&hist_bins[(int)d], 1);  // (-inf: d = +inf, skipped)
    }
  }
  __syncthreads();
  if (wv == 0) {  // first bin at which the running count reaches k (as in the one-stage form)
    constexpr int PER = SMP_BINS / 64;
    int loc = 0;
#pragma unroll 8
    for (int t_ = 0; t_ < PER; ++t_) loc += hist_bins[lane * PER + ((t_ + lane) & (PER - 1))];
    int pre = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(pre, o, 64);
      if (lane >= o) pre += up;
    }
    const bool hit = pre >= k && pre - loc < k;
    if (__builtin_amdgcn_ballot_w64(hit) == 0ull) {
      if (lane == 0) thr_bin = -1;  // fewer than k finite scores in the slice: all of them are candidates, no bound
    } else if (hit) {
      int cum = pre - loc, tb = lane * PER;
      for (int t_ = 0; t_ < PER; ++t_) {
        cum += hist_bins[lane * PER + t_];
        if (cum >= k) { tb = lane * PER + t_; break; }
      }
      thr_bin = cum <= SMP_LCAP ? tb : -2;  // -2: the threshold bin overflows the slice's list
    }
  }
  __syncthreads();
  const int tb = thr_bin;
  if (tb == -2) {  // (uniform)
    if (tid == 0) { atomicOr(&ws.ovf[b], 1); ws.cand_n[b * SMP_G + g] = 0; ws.lb[b * SMP_G + g] = -INFINITY; }
    return;
  }
  const float lim = tb < 0 ? (float)SMP_BINS : (float)(tb + 1);
  float mymin = INFINITY;
#pragma unroll
  for (int e = 0; e < SMP_E4; ++e) {
    const int i4 = lo4 + tid + e * SMP_T;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float v = v4[e][c];
      if ((gmax - v) * bscale < lim) {
        const int slot = atomicAdd(&list_n, 1);
        if (slot < SMP_LCAP) { lv[slot] = v; li[slot] = 4 * i4 + c; }
        mymin = fminf(mymin, v);
      }
    }
  }
  mymin = -wave_max(-mymin);
  if (lane == 0) rm[wv] = mymin;
  __syncthreads();
  const int n = min(list_n, SMP_LCAP);  // (tb >= 0: list_n = the running count at the threshold bin <= SMP_LCAP; tb < 0: < k <= SMP_CAP)
  for (int t_ = tid; t_ < n; t_ += SMP_T) {
    ws.cand_v[slot0 + t_] = lv[t_];
    ws.cand_i[slot0 + t_] = li[t_];
  }
  if (tid == 0) {
    float m_ = rm[0];
    for (int w_ = 1; w_ < SMP_T / 64; ++w_) m_ = fminf(m_, rm[w_]);
    ws.cand_n[b * SMP_G + g] = n;
    ws.lb[b * SMP_G + g] = tb >= 0 ? m_ : -INFINITY;  // (>= k scores of the slice are >= the smallest collected one)
  }
}

// `pre` (ws.cand_v != nullptr): stage 2 of the two-stage form -- the processors are done and the candidates come from the slices
// SLOTS (tcavt_sample_logits_slots): the bookkeeping is per slot -- step_p, max_new and out_row are arrays [B]; slot b chooses token
// step_p[b] of output row out_row[b] (which is also its Philox row), ends on EOS or when its budget max_new[b] is used up, and a
// finished slot is inert: cur_tok[b] = pad and nothing else of its state is written.  The selection itself is the same code.
// ROWS (tcavt_sample_logits_rows): SLOTS, with the logits row and the workspace indexed by the workgroup b and the state by the slot
// sb = slot_of_row[b] of n_state slots; a row without a slot leaves before it has written anything.
// STOP (tcavt_sample_tokens with rules): a live row -- finished == 0 -- also bans the ending tokens while step < min_new (here only
// in the one-stage form; the slices have done it otherwise), ends on a token of the stop set (the token is kept) or when its last n
// generated tokens equal a stop sequence of length n (never reaching into the prompt: step + 1 >= n), and the thread that sets
// `finished` records finish_reason (EOS 1 > stop token 2 > stop sequence 3 > budget 4) and n_generated = step + 1 at the row's
// out_tokens index.  Everything else of a row's step is as without STOP.
constexpr int SMP_BATCH = 0, SMP_SLOTS = 1, SMP_ROWS = 2;
// REQ (tcavt_sample_tokens_per_request): the row's parameters and minimum come from the request tables, see ReqP.
template <int MODE, bool STOP = false, bool REQ = false>
__global__ __launch_bounds__(SMP_T) void sample_kernel(float* __restrict__ logits, int V, long* __restrict__ history,
                                                       int hist_cap, int* __restrict__ hist_len, typename sample_arg<REQ>::type spa,
                                                       int* __restrict__ step_p, long* __restrict__ cur_tok,
                                                       int* __restrict__ pos, int* __restrict__ finished,
                                                       long* __restrict__ out_tokens, int out_cap, int advance_pos, SliceWs ws,
                                                       int n_samples, const int* __restrict__ max_new,
                                                       const long* __restrict__ out_row, const int* __restrict__ slot_of_row,
                                                       int n_state, StopP sr) {
  constexpr bool SLOTS = MODE != SMP_BATCH;
  __shared__ float cv[SMP_CAP];
  __shared__ int ci[SMP_CAP];
  __shared__ float rv[SMP_T / 64];
  __shared__ int ri[SMP_T / 64];
  __shared__ float rm[SMP_T / 64];
  __shared__ float bestv;
  __shared__ int besti;
  __shared__ int hist_bins[SMP_BINS];
  __shared__ float list_v[SMP_LIST];
  __shared__ __attribute__((aligned(16))) int list_i[SMP_LIST];
  __shared__ int list_n, thr_bin, keep_n;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int sb = b;  // the row's entry of the state arrays
  if constexpr (MODE == SMP_ROWS) {
    sb = slot_of_row[b];
    if (sb < 0 || sb >= n_state) return;  // (uniform)
  }
  [[maybe_unused]] SampleP sp_req;
  const SampleP& sp = params_of(spa, sp_req);
  [[maybe_unused]] const int* req_min = nullptr;  // REQ: the request's own minimum, when the call has them
  if constexpr (REQ) {
    const long r = SLOTS ? out_row[sb] : (long)b;  // (batch form: the entry has checked n_req >= rows)
    if (SLOTS && (r < 0 || r >= (long)spa.n_req)) {  // (uniform) inert: nothing of the row is written
      if (tid == 0 && spa.bad_flag) atomicOr(spa.bad_flag, 1);
      return;
    }
    sp_req = request_params(spa, r);
    if (spa.min_new) req_min = spa.min_new + r;
  }
  float* x = logits + (long)b * V;
  long* hist = history + (long)sb * hist_cap;
  const int hl = min(hist_len[sb], hist_cap);
  const int step = SLOTS ? step_p[sb] : *step_p;
  const bool pre = ws.cand_v != nullptr;
  __shared__ int s_ovf;
  if (pre) {
    if (tid == 0) s_ovf = ws.ovf[b];
    __syncthreads();
    if (tid == 0 && s_ovf) ws.ovf[b] = 0;  // (re-armed for the next call)
  }
  const bool pre_ok = pre && s_ovf == 0;  // (uniform) the slices' candidates are complete
  // ---- before the minimum: no ending token (-inf absorbs the penalty, so the order against the processors below does not matter)
  if constexpr (STOP) {
    int min_new = sr.min_new;
    if constexpr (REQ) {
      if (req_min) min_new = *req_min;
    }
    if (!pre && min_new > 0 && step < min_new && finished[sb] == 0) {  // (uniform)
      if (sr.bitmap) {
        for (int i = tid; i < V; i += SMP_T)
          if ((sr.bitmap[i >> 5] >> (i & 31)) & 1u) x[i] = -INFINITY;
      }
      if (tid == 0 && sp.eos >= 0 && sp.eos < V) x[sp.eos] = -INFINITY;
      __syncthreads();
    }
  }
  // ---- repetition penalty: once per distinct token of the history (scatter semantics of the reference processor)
  if (!pre && sp.rep_penalty != 1.f) {
    // (the history is staged in LDS when it fits: thread i compares its token with all earlier ones)
    const bool in_lds = hl <= SMP_LIST;
    if (in_lds) {
      for (int i = tid; i < hl; i += SMP_T) list_i[i] = (int)min(max(hist[i], -1L), 0x7fffffffL);  // (ids >= 2^31 - 1 are out of range anyway)
      __syncthreads();
    }
    for (int i = tid; i < hl; i += SMP_T) {
      const long t = hist[i];
      bool first = t >= 0 && t < V;
      if (in_lds) {
        first = first && !occurs_before(list_i, i, (int)t);
      } else {
        for (int j = 0; j < i && first; ++j) first = hist[j] != t;
      }
      if (first) {
        const float s = x[t];
        x[t] = s < 0.f ? s * sp.rep_penalty : s / sp.rep_penalty;
      }
    }
    __syncthreads();
  }
  // ---- no-repeat n-gram: ban every token that would complete an n-gram already in the history
  const int ng = sp.no_repeat_ngram;
  if (!pre && ng > 0 && hl + 1 >= ng) {
    for (int i = tid; i + ng - 1 < hl; i += SMP_T) {
      bool match = true;
      for (int k = 0; k < ng - 1 && match; ++k) match = hist[i + k] == hist[hl - (ng - 1) + k];
      const long t = hist[i + ng - 1];
      if (match && t >= 0 && t < V) x[t] = -INFINITY;
    }
    __syncthreads();
  }
  // every logit of the sample, 16 bytes per lane and load when the row allows (V % 4 == 0, aligned) and several loads in flight:
  // the passes below are latency bound (one workgroup per sample), so fewer and wider loads are what shortens them
  auto walk = [&](auto&& f) {
    if ((V & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
      const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
      const int V4 = V >> 2;
#pragma unroll 4
      for (int i4 = tid; i4 < V4; i4 += SMP_T) {
        const f32x4 t = x4[i4];
        f(t[0], 4 * i4);
        f(t[1], 4 * i4 + 1);
        f(t[2], 4 * i4 + 2);
        f(t[3], 4 * i4 + 3);
      }
    } else {
#pragma unroll 4
      for (int i = tid; i < V; i += SMP_T) f(x[i], i);
    }
  };
  // block-wide arg-max of the elements that come after (pv, pi) in (value desc, index asc) order; with_min: also the
  // smallest finite value (left in rv[0] region -> minv) in the same pass
  __shared__ float minv;
  auto next_best = [&](float pv, int pi, float scale, bool with_min) {
    float bv = -INFINITY, lmin = INFINITY;
    int bi = 0x7fffffff;
    walk([&](float raw, int i) {
      const float v = raw * scale;
      if (after(v, i, pv, pi) && better(v, i, bv, bi)) { bv = v; bi = i; }
      if (with_min && v > -INFINITY) lmin = fminf(lmin, v);
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (with_min) lmin = -wave_max(-lmin);
    if (lane == 0) { rv[wv] = bv; ri[wv] = bi; rm[wv] = lmin; }
    __syncthreads();
    if (tid == 0) {
      float v = rv[0], m_ = rm[0];
      int i = ri[0];
      for (int k = 1; k < SMP_T / 64; ++k) {
        if (better(rv[k], ri[k], v, i)) { v = rv[k]; i = ri[k]; }
        m_ = fminf(m_, rm[k]);
      }
      bestv = v;
      besti = i;
      minv = m_;
    }
    __syncthreads();
  };
  long tok;
  if (!sp.do_sample && pre_ok) {  // greedy, two-stage form: the best of the slices' first maxima
    if (tid < 64) {
      float bv = -INFINITY;
      int bi = 0x7fffffff;
      if (tid < SMP_G && ws.cand_n[b * SMP_G + tid] > 0) {
        bv = ws.cand_v[((long)b * SMP_G + tid) * SMP_LCAP];
        bi = ws.cand_i[((long)b * SMP_G + tid) * SMP_LCAP];
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
      }
      if (tid == 0) besti = bi;
    }
    __syncthreads();
    tok = besti;
  } else if (!sp.do_sample) {  // greedy: arg-max of the processed scores, first maximum wins (torch.argmax)
    next_best(INFINITY, -1, 1.f, false);
    tok = besti;
  } else {
    // Candidate collection in three passes over the vocabulary instead of one pass per candidate: (1) the maximum and the
    // minimum (one pass), (2) a histogram of (max - score) in SMP_BINS bins over that range (integer counts: order-independent), from which the narrowest
    // threshold that keeps at least top_k scores follows, (3) everything at or above that threshold goes to an LDS list
    // (top_k + the rest of the threshold bin; insertion order does not matter, the selection below orders by
    // (value, index)).  The list is then ordered by top_k rounds of a wave-level arg-max over <= SMP_LIST entries.
    const float invT = 1.f / sp.temperature;
    const int k = min(max(sp.top_k, 1), SMP_CAP);
    bool have_list = false;  // (uniform)
    if (pre_ok) {
      // two-stage form: every slice's candidates at or above the largest of the slices' bounds (>= k scores of ONE slice lie at
      // or above its bound, so the sample's k-th largest score does too: nothing below it can be kept)
      if (tid == 0) { list_n = 0; keep_n = 0; }
      // (one slice per WAVE -- SMP_G == SMP_T / 64 -- and every load of a phase in flight together: written as a loop over the
      //  slices this was 2 x 16 dependent round trips to memory that another CU has just written, 40 us for a ~10 us kernel)
      static_assert(SMP_G == SMP_T / 64, "one wave per slice");
      float lmax = ws.lb[b * SMP_G + (lane & (SMP_G - 1))];
#pragma unroll
      for (int o = 1; o < SMP_G; o <<= 1) lmax = fmaxf(lmax, __shfl_xor(lmax, o, 64));
      const int n_g = ws.cand_n[b * SMP_G + wv];
      const long s0 = ((long)b * SMP_G + wv) * SMP_LCAP;
      float cvv[SMP_LCAP / 64];
      int cii[SMP_LCAP / 64];
#pragma unroll
      for (int e = 0; e < SMP_LCAP / 64; ++e) {
        const int t_ = lane + 64 * e;
        cvv[e] = t_ < n_g ? ws.cand_v[s0 + t_] : -INFINITY;
        cii[e] = t_ < n_g ? ws.cand_i[s0 + t_] : 0;
      }
      __syncthreads();
#pragma unroll
      for (int e = 0; e < SMP_LCAP / 64; ++e) {
        if (lane + 64 * e < n_g && cvv[e] >= lmax) {
          const int slot = atomicAdd(&list_n, 1);
          if (slot < SMP_LIST) { list_v[slot] = cvv[e]; list_i[slot] = cii[e]; }
        }
      }
      __syncthreads();
      have_list = list_n <= SMP_LIST;  // (more: the three passes below, over the already processed logits)
      if (tid == 0 && have_list) thr_bin = 0;
      __syncthreads();
    }
    float gmax = 0.f, bscale = 0.f;
    if (!have_list) {
    next_best(INFINITY, -1, invT, true);  // (1): the maximum and, in the same pass, the smallest finite score
    gmax = bestv;
    // bin width from the spread of the finite scores: SMP_BINS bins between the maximum and the minimum
    bscale = (float)(SMP_BINS - 1) / fmaxf(gmax - minv, 1e-20f);
    __syncthreads();
    for (int i = tid; i < SMP_BINS; i += SMP_T) hist_bins[i] = 0;
    if (tid == 0) { list_n = 0; keep_n = 0; }
    __syncthreads();
    walk([&](float raw, int) {
      const float d = (gmax - raw * invT) * bscale;
      if (d < (float)SMP_BINS) atomicAdd(&hist_bins[(int)d], 1);  // (-inf scores: d = +inf, skipped)
    });
    __syncthreads();
    if (wv == 0) {
      // first bin at which the running count reaches k: every lane adds up its SMP_BINS / 64 consecutive bins, a wave scan
      // finds the lane in whose range the count crosses k, and only that lane walks its bins (one thread walking all 2048
      // bins was a chain of up to 2048 dependent LDS reads)
      constexpr int PER = SMP_BINS / 64;
      int loc = 0;
#pragma unroll 8
      for (int t_ = 0; t_ < PER; ++t_) loc += hist_bins[lane * PER + ((t_ + lane) & (PER - 1))];  // (rotated: 2-way instead of 64-way bank conflicts)
      int pre = loc;  // inclusive prefix over the lanes
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(pre, o, 64);
        if (lane >= o) pre += up;
      }
      const bool hit = pre >= k && pre - loc < k;
      if (__builtin_amdgcn_ballot_w64(hit) == 0ull) {
        if (lane == 0) thr_bin = -1;  // fewer than k scores in range -> exact fallback
      } else if (hit) {
        int cum = pre - loc, tb = lane * PER;
        for (int t_ = 0; t_ < PER; ++t_) {
          cum += hist_bins[lane * PER + t_];
          if (cum >= k) { tb = lane * PER + t_; break; }
        }
        thr_bin = cum <= SMP_LIST ? tb : -1;  // -1: too many scores in the threshold bin -> exact fallback
      }
    }
    __syncthreads();
    }  // (!have_list)
    int n = 0;
    if (thr_bin >= 0) {
      if (!have_list) {
        const float lim = (float)(thr_bin + 1);
        walk([&](float raw, int i) {
          const float v = raw * invT;
          if ((gmax - v) * bscale < lim) {
            const int slot = atomicAdd(&list_n, 1);
            if (slot < SMP_LIST) { list_v[slot] = v; list_i[slot] = i; }
          }
        });
        __syncthreads();
      }
      const int ln = min(list_n, SMP_LIST);
      // order the list by RANK: entry t precedes rank(t) others in (value desc, index asc) order -- indices are distinct, so
      // the ranks are a permutation -- and goes to slot rank(t).  Every thread reads the same list entry at a time (LDS
      // broadcast).  Kept: the first k and every tie with the k-th value (as `scores < topk[-1]` keeps them), capped at
      // SMP_CAP.  (The first version picked the next entry by a wave-wide arg-max, one round per candidate.)
      float mv = 0.f;
      int mi = 0, rank = 0x7fffffff;
      if (tid < ln) {
        mv = list_v[tid];
        mi = list_i[tid];
        rank = 0;
        for (int j = 0; j < ln; ++j) rank += better(list_v[j], list_i[j], mv, mi) ? 1 : 0;
        if (rank < SMP_CAP) { cv[rank] = mv; ci[rank] = mi; }
      }
      __syncthreads();
      const int kk = min(k, ln);
      if (tid < ln && kk > 0 && (rank < kk || mv == cv[kk - 1])) atomicAdd(&keep_n, 1);
      __syncthreads();
      n = min(keep_n, SMP_CAP);
    } else {  // exact fallback: one pass over the vocabulary per candidate
      float pv = INFINITY;
      int pi = -1;
      for (;;) {
        next_best(pv, pi, invT, false);
        const float v = bestv;
        const int i = besti;
        if (i == 0x7fffffff || v == -INFINITY) break;        // nothing (finite) left
        if (n >= k && !(v == cv[k - 1])) break;               // beyond top-k and not a tie with the k-th value
        if (n >= SMP_CAP) break;
        if (tid == 0) { cv[n] = v; ci[n] = i; }
        ++n;
        pv = v;
        pi = i;
        __syncthreads();
      }
    }
    if (tid == 0) {
      // softmax over the kept candidates (descending), top-p: drop the low tail whose cumulative probability, counted
      // from the bottom and including the item, is <= 1 - top_p (keep at least one)
      const float m = cv[0];
      float tot = 0.f;
      for (int j = 0; j < n; ++j) tot += __expf(cv[j] - m);
      int keep = n;
      if (sp.top_p < 1.f) {
        float tail = 0.f;
        for (int j = n - 1; j >= 1; --j) {
          tail += __expf(cv[j] - m) / tot;
          if (tail <= 1.f - sp.top_p) keep = j;
          else break;
        }
      }
      float kt = 0.f;
      for (int j = 0; j < keep; ++j) kt += __expf(cv[j] - m);
      unsigned int r[4];
      philox4x32_10((unsigned int)step, SLOTS ? (unsigned int)out_row[sb] : (unsigned int)b, 0x5A3Bu, 0u, sp.seed_lo, sp.seed_hi, r);
      const float u = (float)(r[0] >> 8) * (1.0f / 16777216.0f) * kt;
      float acc = 0.f;
      int pick = keep - 1;
      for (int j = 0; j < keep; ++j) {
        acc += __expf(cv[j] - m);
        if (u < acc) { pick = j; break; }
      }
      besti = n > 0 ? ci[pick] : 0;
    }
    __syncthreads();
    tok = besti;
  }
  // ---- stop sequences: thread (q, j) compares element j from the end of sequence q with the j-th newest generated token (the new
  // token, then history elements hl - 1 ...); one predicated load each, no data-dependent trip count; a sequence matches when its
  // eight lanes agree (lanes past its length agree by definition)
  bool seq_hit = false;
  if constexpr (STOP) {
    __shared__ int s_seq[2];
    static_assert(SMP_SEQS * SMP_SEQ_LEN == 128 && SMP_SEQ_LEN == 8, "two waves, one sequence per 8 lanes");
    if (sr.n_seqs > 0) {  // (uniform)
      if (tid < SMP_SEQS * SMP_SEQ_LEN) {
        const int q = tid >> 3, j = tid & 7;
        bool ok = false;
        if (q < sr.n_seqs) {
          const int len = sr.seq_len[q];
          const bool len_ok = len >= 1 && len <= SMP_SEQ_LEN && step + 1 >= len;
          const int lc = len_ok ? len : 1;
          const bool mine = j < lc;
          const long want = sr.seqs[q * SMP_SEQ_LEN + (mine ? lc - 1 - j : 0)];
          const bool there = j == 0 || hl - j >= 0;  // (only history elements that exist)
          const long have = j == 0 ? tok : (there ? hist[hl - j] : -1L);
          ok = len_ok && (!mine || (there && have == want));
        }
        unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
        m &= m >> 1; m &= m >> 2; m &= m >> 4;
        if (lane == 0) s_seq[wv] = (m & 0x0101010101010101ull) != 0ull;
      }
      __syncthreads();
      seq_hit = (s_seq[0] | s_seq[1]) != 0;
    }
  }
  // how a live row ends on `tok` (0: it does not), budget aside
  auto end_reason = [&]() -> int {
    if (sp.eos >= 0 && tok == sp.eos) return FIN_EOS;
    if (sr.bitmap && tok >= 0 && tok < V && ((sr.bitmap[tok >> 5] >> (tok & 31)) & 1u)) return FIN_STOP_TOKEN;
    return seq_hit ? FIN_STOP_SEQ : 0;
  };
  auto record = [&](long row, int reason) {
    if (sr.finish_reason) sr.finish_reason[row] = reason;
    if (sr.n_generated) sr.n_generated[row] = step + 1;
  };
  if constexpr (SLOTS) {
    if (tid == 0) {
      if (finished[sb] != 0) {  // inert: the decode step keeps running this slot on the pad token at its frozen position
        cur_tok[sb] = sp.pad;
      } else {
        if (step < out_cap) out_tokens[out_row[sb] * out_cap + step] = tok;
        cur_tok[sb] = tok;
        if (hl < hist_cap) {
          hist[hl] = tok;
          hist_len[sb] = hl + 1;
        }
        if (advance_pos) pos[sb] += 1;
        if constexpr (STOP) {
          int reason = end_reason();
          if (!reason && step + 1 == max_new[sb]) reason = FIN_BUDGET;
          if (reason) {
            finished[sb] = 1;
            record(out_row[sb], reason);
          }
        } else {
          if ((sp.eos >= 0 && tok == sp.eos) || step + 1 == max_new[sb]) finished[sb] = 1;
        }
        step_p[sb] = step + 1;  // (the slot's own word: no ticket)
      }
    }
    return;
  }
  if (tid == 0) {
    // a finished sample keeps emitting the pad token (HF generate pads finished rows)
    const bool fin = finished[b] != 0;
    const long outt = fin ? sp.pad : tok;
    if (step < out_cap) out_tokens[(long)b * out_cap + step] = outt;
    if constexpr (STOP) {
      const int reason = fin ? 0 : end_reason();
      if (reason) {
        finished[b] = 1;
        record(b, reason);
      }
    } else {
      if (!fin && sp.eos >= 0 && tok == sp.eos) finished[b] = 1;
    }
    cur_tok[b] = outt;
    if (hl < hist_cap) {
      hist[hl] = outt;
      hist_len[b] = hl + 1;
    }
    if (advance_pos) pos[b] += 1;
  }
  if (pre && tid == 0) {
    // *step is advanced here instead of by a launch of its own: every workgroup has read it by the time it takes its ticket,
    // and the one that draws the last ticket writes step + 1 and re-arms the counter
    const int t_ = __hip_atomic_fetch_add(ws.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t_ == n_samples - 1) {
      __hip_atomic_store(ws.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *step_p = step + 1;
    }
  }
}

__global__ void step_inc_kernel(int* step) { *step += 1; }

}  // namespace tcavt

using namespace tcavt;

extern "C" int64_t tcavt_sample_workspace_bytes(int B) {
  if (B <= 0) return 0;
  return 64 + (((int64_t)B * 4 + 63) & ~(int64_t)63) + (int64_t)B * SMP_G * 8 + (int64_t)B * SMP_G * SMP_LCAP * 8;
}

// tcavt_sample_logits (max_new == out_row == NULL, one step word), tcavt_sample_logits_slots (arrays [B]) and tcavt_sample_logits_rows
// (slot_of_row: B logits rows on the state of n_state slots) share the launches
static int sample_logits_impl(const char* who, float* logits, int B, int V, const int32_t* slot_of_row, int n_state, int64_t* history,
                              int hist_cap, int32_t* hist_len, const tcavt_sample_params* sp, int32_t* step, const int32_t* max_new, const int64_t* out_row, int64_t* cur_tok,
                              int32_t* pos, int32_t* finished, int64_t* out_tokens, int out_cap, int advance_pos, void* workspace,
                              int64_t workspace_bytes, tcavt_stream_t stream, const tcavt_stop_rules* rules = nullptr,
                              const tcavt_request_params* req = nullptr) {
  const bool slots = max_new || out_row;
  // ending rules: with none set (or rules == NULL) the launches below are the instantiations without STOP, argument for argument
  StopP sr = {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
  bool stop = false;
  if (rules) {
    TCAVT_CHECK_ARG(rules->n_seqs >= 0 && rules->n_seqs <= SMP_SEQS, "%s: stop rules: n_seqs = %d outside [0, %d]", who, rules->n_seqs, SMP_SEQS);
    TCAVT_CHECK_ARG(rules->n_seqs == 0 || rules->stop_seqs, "%s: stop rules: stop_seqs is a null pointer with n_seqs = %d", who, rules->n_seqs);
    TCAVT_CHECK_ARG(rules->n_seqs == 0 || rules->stop_seq_len, "%s: stop rules: stop_seq_len is a null pointer with n_seqs = %d", who, rules->n_seqs);
    TCAVT_CHECK_ARG(rules->min_new_tokens >= 0, "%s: stop rules: min_new_tokens = %d must be >= 0", who, rules->min_new_tokens);
    TCAVT_CHECK_ARG(rules->min_new_tokens == 0 || sp->eos_token_id >= 0 || rules->stop_bitmap,
                    "%s: stop rules: min_new_tokens = %d with neither eos_token_id nor stop_bitmap (nothing to ban)", who, rules->min_new_tokens);
    TCAVT_CHECK_ARG((reinterpret_cast<uintptr_t>(rules->stop_bitmap) & 3) == 0, "%s: stop rules: stop_bitmap must be 4-byte aligned", who);
    sr.bitmap = rules->stop_bitmap;
    sr.seqs = rules->n_seqs > 0 ? reinterpret_cast<const long*>(rules->stop_seqs) : nullptr;
    sr.seq_len = rules->n_seqs > 0 ? rules->stop_seq_len : nullptr;
    sr.finish_reason = rules->finish_reason; sr.n_generated = rules->n_generated;
    sr.n_seqs = rules->n_seqs; sr.min_new = rules->min_new_tokens;
    stop = sr.bitmap || sr.n_seqs > 0 || sr.min_new > 0 || sr.finish_reason || sr.n_generated;
  }
  // per-request parameters: the REQ instantiations, argument for argument the launches below with the tables in the struct's place
  ReqP rq = {nullptr, nullptr, nullptr, nullptr, 0, 0};
  if (req) {
    TCAVT_CHECK_ARG(req->table, "%s: request params: table is a null pointer", who);
    TCAVT_CHECK_ARG(req->n_req >= 1, "%s: request params: n_req = %d must be >= 1", who, req->n_req);
    TCAVT_CHECK_ARG(slots || req->n_req >= B, "%s: request params: n_req = %d is below rows = %d (batch form: the request of row b is b)",
                    who, req->n_req, B);
    TCAVT_CHECK_ARG((reinterpret_cast<uintptr_t>(req->table) & 7) == 0, "%s: request params: table must be 8-byte aligned", who);
    TCAVT_CHECK_ARG((reinterpret_cast<uintptr_t>(req->min_new_tokens) & 3) == 0, "%s: request params: min_new_tokens must be 4-byte aligned", who);
    TCAVT_CHECK_ARG((reinterpret_cast<uintptr_t>(req->bad_index_flag) & 3) == 0, "%s: request params: bad_index_flag must be 4-byte aligned", who);
    rq.table = req->table; rq.min_new = req->min_new_tokens; rq.bad_flag = req->bad_index_flag;
    rq.out_row = slots ? reinterpret_cast<const long*>(out_row) : nullptr;
    rq.pad = sp->pad_token_id; rq.n_req = req->n_req;
    stop = stop || rq.min_new;  // (a request's own minimum needs the ban of the STOP forms)
  }
  TCAVT_CHECK_ARG(!sp->do_sample || (sp->temperature > 0.f && sp->top_k >= 1 && sp->top_k <= SMP_CAP && sp->top_p > 0.f && sp->top_p <= 1.f),
                  "%s: sampling needs temperature > 0, 1 <= top_k <= %d, 0 < top_p <= 1", who, SMP_CAP);
  TCAVT_CHECK_ARG(sp->repetition_penalty > 0.f && sp->no_repeat_ngram_size >= 0, "%s: bad repetition_penalty / no_repeat_ngram_size", who);
  SampleP p;
  p.temperature = sp->temperature; p.top_p = sp->top_p; p.rep_penalty = sp->repetition_penalty;
  p.top_k = sp->top_k; p.no_repeat_ngram = sp->no_repeat_ngram_size; p.do_sample = sp->do_sample;
  p.eos = sp->eos_token_id; p.pad = sp->pad_token_id;
  p.seed_lo = (unsigned int)(sp->seed & 0xffffffffu); p.seed_hi = (unsigned int)(sp->seed >> 32);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // two-stage form when the caller lends a workspace and the rows can be cut into 16-byte-aligned slices that fit the registers
  SliceWs ws = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const int64_t need = tcavt_sample_workspace_bytes(B);
  const int chunk4 = ((V >> 2) + SMP_G - 1) / SMP_G;
  if (workspace && workspace_bytes >= need && (V & 3) == 0 && aligned16(logits) && chunk4 <= SMP_E4 * SMP_T) {
    TCAVT_CHECK_ARG(aligned16(workspace), "%s: workspace must be 16-byte aligned", who);
    char* w = static_cast<char*>(workspace);
    ws.ticket = reinterpret_cast<int*>(w);
    ws.ovf = reinterpret_cast<int*>(w + 64);
    size_t off = 64 + (((size_t)B * 4 + 63) & ~(size_t)63);
    ws.cand_n = reinterpret_cast<int*>(w + off); off += (size_t)B * SMP_G * 4;
    ws.lb = reinterpret_cast<float*>(w + off); off += (size_t)B * SMP_G * 4;
    ws.cand_v = reinterpret_cast<float*>(w + off); off += (size_t)B * SMP_G * SMP_LCAP * 4;
    ws.cand_i = reinterpret_cast<int*>(w + off);
    if (req) {
      auto* skern = sample_slice_kernel<false, true>;
      if (stop) skern = sample_slice_kernel<true, true>;
      hipLaunchKernelGGL(skern, dim3(B * SMP_G), dim3(SMP_T), 0, st, logits, V, reinterpret_cast<const long*>(history), hist_cap, hist_len,
                         rq, ws, slot_of_row, n_state, sr, step, slots ? 1 : 0, finished);
    } else {
      hipLaunchKernelGGL(stop ? sample_slice_kernel<true> : sample_slice_kernel<false>, dim3(B * SMP_G), dim3(SMP_T), 0, st, logits, V,
                         reinterpret_cast<const long*>(history), hist_cap, hist_len, p, ws, slot_of_row, n_state, sr, step, slots ? 1 : 0, finished);
    }
  }
  if (req) {
    auto* rkern = slot_of_row ? sample_kernel<SMP_ROWS, false, true> : slots ? sample_kernel<SMP_SLOTS, false, true> : sample_kernel<SMP_BATCH, false, true>;
    if (stop) rkern = slot_of_row ? sample_kernel<SMP_ROWS, true, true> : slots ? sample_kernel<SMP_SLOTS, true, true> : sample_kernel<SMP_BATCH, true, true>;
    hipLaunchKernelGGL(rkern, dim3(B), dim3(SMP_T),
                       0, st, logits, V, reinterpret_cast<long*>(history), hist_cap, hist_len, rq, step, reinterpret_cast<long*>(cur_tok), pos,
                       finished, reinterpret_cast<long*>(out_tokens), out_cap, advance_pos, ws, B, max_new,
                       reinterpret_cast<const long*>(out_row), slot_of_row, n_state, sr);
    if (!ws.cand_v && !slots) hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, st, step);
    TCAVT_CHECK_LAUNCH(who);
    return TCAVT_OK;
  }
  auto* kern = slot_of_row ? sample_kernel<SMP_ROWS> : slots ? sample_kernel<SMP_SLOTS> : sample_kernel<SMP_BATCH>;
  if (stop) kern = slot_of_row ? sample_kernel<SMP_ROWS, true> : slots ? sample_kernel<SMP_SLOTS, true> : sample_kernel<SMP_BATCH, true>;
  hipLaunchKernelGGL(kern, dim3(B), dim3(SMP_T),
                     0, st, logits, V, reinterpret_cast<long*>(history), hist_cap, hist_len, p, step, reinterpret_cast<long*>(cur_tok), pos,
                     finished, reinterpret_cast<long*>(out_tokens), out_cap, advance_pos, ws, B, max_new,
                     reinterpret_cast<const long*>(out_row), slot_of_row, n_state, sr);
  if (!ws.cand_v && !slots) hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, st, step);
  TCAVT_CHECK_LAUNCH(who);
  return TCAVT_OK;
}

extern "C" int tcavt_sample_logits(float* logits, int B, int V, int64_t* history, int hist_cap, int32_t* hist_len,
                                   const tcavt_sample_params* sp, int32_t* step, int64_t* cur_tok, int32_t* pos,
                                   int32_t* finished, int64_t* out_tokens, int out_cap, int advance_pos, void* workspace,
                                   int64_t workspace_bytes, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(logits && history && hist_len && sp && step && cur_tok && pos && finished && out_tokens && B > 0 && V > 0 &&
                      hist_cap > 0 && out_cap > 0,
                  "sample_logits: bad args");
  return sample_logits_impl("sample_logits", logits, B, V, nullptr, B, history, hist_cap, hist_len, sp, step, nullptr, nullptr, cur_tok, pos, finished,
                            out_tokens, out_cap, advance_pos, workspace, workspace_bytes, stream);
}

extern "C" int tcavt_sample_logits_slots(float* logits, int S, int V, int64_t* history, int hist_cap, int32_t* hist_len,
                                         const tcavt_sample_params* sp, int32_t* step, const int32_t* max_new, const int64_t* out_row,
                                         int64_t* cur_tok, int32_t* pos, int32_t* finished, int64_t* out_tokens, int out_cap,
                                         int advance_pos, void* workspace, int64_t workspace_bytes, tcavt_stream_t stream) {
  const struct { const void* p; const char* name; } ptrs[] = {
      {logits, "logits"}, {history, "history"}, {hist_len, "hist_len"}, {sp, "params"}, {step, "step"}, {max_new, "max_new"},
      {out_row, "out_row"}, {cur_tok, "cur_tok"}, {pos, "pos"}, {finished, "finished"}, {out_tokens, "out_tokens"}};
  for (const auto& a : ptrs) TCAVT_CHECK_ARG(a.p, "sample_logits_slots: %s is a null pointer", a.name);
  TCAVT_CHECK_ARG(S > 0, "sample_logits_slots: S = %d must be > 0", S);
  TCAVT_CHECK_ARG(V > 0, "sample_logits_slots: V = %d must be > 0", V);
  TCAVT_CHECK_ARG(hist_cap > 0, "sample_logits_slots: hist_cap = %d must be > 0", hist_cap);
  TCAVT_CHECK_ARG(out_cap > 0, "sample_logits_slots: out_cap = %d must be > 0", out_cap);
  return sample_logits_impl("sample_logits_slots", logits, S, V, nullptr, S, history, hist_cap, hist_len, sp, step, max_new, out_row, cur_tok, pos,
                            finished, out_tokens, out_cap, advance_pos, workspace, workspace_bytes, stream);
}

extern "C" int tcavt_sample_logits_rows(float* logits, int G, int V, const int32_t* slot_of_row, int S, int64_t* history, int hist_cap,
                                        int32_t* hist_len, const tcavt_sample_params* sp, int32_t* step, const int32_t* max_new,
                                        const int64_t* out_row, int64_t* cur_tok, int32_t* pos, int32_t* finished, int64_t* out_tokens,
                                        int out_cap, int advance_pos, void* workspace, int64_t workspace_bytes, tcavt_stream_t stream) {
  const struct { const void* p; const char* name; } ptrs[] = {
      {logits, "logits"}, {slot_of_row, "slot_of_row"}, {history, "history"}, {hist_len, "hist_len"}, {sp, "params"}, {step, "step"},
      {max_new, "max_new"}, {out_row, "out_row"}, {cur_tok, "cur_tok"}, {pos, "pos"}, {finished, "finished"}, {out_tokens, "out_tokens"}};
  for (const auto& a : ptrs) TCAVT_CHECK_ARG(a.p, "sample_logits_rows: %s is a null pointer", a.name);
  TCAVT_CHECK_ARG(G > 0, "sample_logits_rows: G = %d must be > 0", G);
  TCAVT_CHECK_ARG(S > 0, "sample_logits_rows: S = %d must be > 0", S);
  TCAVT_CHECK_ARG(V > 0, "sample_logits_rows: V = %d must be > 0", V);
  TCAVT_CHECK_ARG(hist_cap > 0, "sample_logits_rows: hist_cap = %d must be > 0", hist_cap);
  TCAVT_CHECK_ARG(out_cap > 0, "sample_logits_rows: out_cap = %d must be > 0", out_cap);
  return sample_logits_impl("sample_logits_rows", logits, G, V, slot_of_row, S, history, hist_cap, hist_len, sp, step, max_new, out_row,
                            cur_tok, pos, finished, out_tokens, out_cap, advance_pos, workspace, workspace_bytes, stream);
}

extern "C" int tcavt_sample_tokens(const tcavt_sample_args* a, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(a, "sample_tokens: args is a null pointer");
  const bool rows = a->slot_of_row != nullptr, slots = rows || a->max_new || a->out_row;
  const struct { const void* p; const char* name; bool need; } ptrs[] = {
      {a->logits, "logits", true}, {a->history, "history", true}, {a->hist_len, "hist_len", true}, {a->params, "params", true},
      {a->step, "step", true}, {a->max_new, "max_new", slots}, {a->out_row, "out_row", slots}, {a->cur_tok, "cur_tok", true},
      {a->pos, "pos", true}, {a->finished, "finished", true}, {a->out_tokens, "out_tokens", true}};
  for (const auto& q : ptrs) TCAVT_CHECK_ARG(q.p || !q.need, "sample_tokens: %s is a null pointer", q.name);
  TCAVT_CHECK_ARG(a->rows > 0, "sample_tokens: rows = %d must be > 0", a->rows);
  TCAVT_CHECK_ARG(a->V > 0, "sample_tokens: V = %d must be > 0", a->V);
  TCAVT_CHECK_ARG(!rows || a->n_state > 0, "sample_tokens: n_state = %d must be > 0 with slot_of_row", a->n_state);
  TCAVT_CHECK_ARG(a->hist_cap > 0, "sample_tokens: hist_cap = %d must be > 0", a->hist_cap);
  TCAVT_CHECK_ARG(a->out_cap > 0, "sample_tokens: out_cap = %d must be > 0", a->out_cap);
  return sample_logits_impl("sample_tokens", a->logits, a->rows, a->V, a->slot_of_row, rows ? a->n_state : a->rows, a->history, a->hist_cap,
                            a->hist_len, a->params, a->step, a->max_new, a->out_row, a->cur_tok, a->pos, a->finished, a->out_tokens,
                            a->out_cap, a->advance_pos, a->workspace, a->workspace_bytes, stream, a->stop);
}

// tcavt_sample_tokens with the parameters per request: the same pointer rules, then the REQ launches
extern "C" int tcavt_sample_tokens_per_request(const tcavt_sample_args* a, const tcavt_request_params* req, tcavt_stream_t stream) {
  const char* who = "sample_tokens_per_request";
  TCAVT_CHECK_ARG(a, "%s: args is a null pointer", who);
  TCAVT_CHECK_ARG(req, "%s: request params is a null pointer", who);
  const bool rows = a->slot_of_row != nullptr, slots = rows || a->max_new || a->out_row;
  const struct { const void* p; const char* name; bool need; } ptrs[] = {
      {a->logits, "logits", true}, {a->history, "history", true}, {a->hist_len, "hist_len", true}, {a->params, "params", true},
      {a->step, "step", true}, {a->max_new, "max_new", slots}, {a->out_row, "out_row", slots}, {a->cur_tok, "cur_tok", true},
      {a->pos, "pos", true}, {a->finished, "finished", true}, {a->out_tokens, "out_tokens", true}};
  for (const auto& q : ptrs) TCAVT_CHECK_ARG(q.p || !q.need, "%s: %s is a null pointer", who, q.name);
  TCAVT_CHECK_ARG(a->rows > 0, "%s: rows = %d must be > 0", who, a->rows);
  TCAVT_CHECK_ARG(a->V > 0, "%s: V = %d must be > 0", who, a->V);
  TCAVT_CHECK_ARG(!rows || a->n_state > 0, "%s: n_state = %d must be > 0 with slot_of_row", who, a->n_state);
  TCAVT_CHECK_ARG(a->hist_cap > 0, "%s: hist_cap = %d must be > 0", who, a->hist_cap);
  TCAVT_CHECK_ARG(a->out_cap > 0, "%s: out_cap = %d must be > 0", who, a->out_cap);
  return sample_logits_impl(who, a->logits, a->rows, a->V, a->slot_of_row, rows ? a->n_state : a->rows, a->history, a->hist_cap,
                            a->hist_len, a->params, a->step, a->max_new, a->out_row, a->cur_tok, a->pos, a->finished, a->out_tokens,
                            a->out_cap, a->advance_pos, a->workspace, a->workspace_bytes, stream, a->stop, req);
}

// the checks sample_logits_impl makes on the one struct, on every entry of a HOST table (no device needed)
extern "C" int tcavt_request_params_check(const tcavt_sample_params* t, const int32_t* min_new, int n_req, int has_stop_bitmap) {
  const char* who = "request_params_check";
  TCAVT_CHECK_ARG(t, "%s: host_table is a null pointer", who);
  TCAVT_CHECK_ARG(n_req >= 1, "%s: n_req = %d must be >= 1", who, n_req);
  for (int r = 0; r < n_req; ++r) {
    const tcavt_sample_params& p = t[r];
    if (p.do_sample) {
      TCAVT_CHECK_ARG(p.temperature > 0.f, "%s: table[%d].temperature = %g must be > 0 when sampling", who, r, (double)p.temperature);
      TCAVT_CHECK_ARG(p.top_k >= 1 && p.top_k <= SMP_CAP, "%s: table[%d].top_k = %d outside [1, %d] when sampling", who, r, p.top_k, SMP_CAP);
      TCAVT_CHECK_ARG(p.top_p > 0.f && p.top_p <= 1.f, "%s: table[%d].top_p = %g outside (0, 1] when sampling", who, r, (double)p.top_p);
    }
    TCAVT_CHECK_ARG(p.repetition_penalty > 0.f, "%s: table[%d].repetition_penalty = %g must be > 0", who, r, (double)p.repetition_penalty);
    TCAVT_CHECK_ARG(p.no_repeat_ngram_size >= 0, "%s: table[%d].no_repeat_ngram_size = %d must be >= 0", who, r, p.no_repeat_ngram_size);
    TCAVT_CHECK_ARG(p.pad_token_id == t[0].pad_token_id, "%s: table[%d].pad_token_id = %lld differs from table[0].pad_token_id = %lld (one per call)",
                    who, r, (long long)p.pad_token_id, (long long)t[0].pad_token_id);
    if (min_new) {
      TCAVT_CHECK_ARG(min_new[r] >= 0, "%s: min_new_tokens[%d] = %d must be >= 0", who, r, min_new[r]);
      TCAVT_CHECK_ARG(min_new[r] == 0 || p.eos_token_id >= 0 || has_stop_bitmap,
                      "%s: min_new_tokens[%d] = %d with neither table[%d].eos_token_id nor a stop bitmap (nothing to ban)", who, r, min_new[r], r);
    }
  }
  return TCAVT_OK;
}
