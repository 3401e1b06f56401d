// Prompt-lookup speculative decoding (include/tcavt.h: tcavt_ngram_draft, tcavt_spec_verify): the two launches that stand around the
// multi-position decode step (csrc/generate.hip: tcavt_llama_decode_step_multi).  The draft of a sequence is the continuation of the
// earliest earlier occurrence of its last n ids (HF PromptLookupCandidateGenerator); the verification selects the token of every
// position with the plain sampler on the state the plain loop would have there, and commits while the selection equals the draft.
#include "common.hpp"

namespace tcavt {

constexpr int DRAFT_T = 256;  // threads of a draft workgroup (and the limit of k + 1)

// One workgroup per sequence.  The history is read where it lies, as int64: it is a few hundred ids, every thread tests the windows
// i = tid, tid + 256, .. against the last n ids, and nothing is staged or narrowed, so ids outside [0, 2^31) compare as themselves.
// The window at i = len - n is the n-gram itself (its continuation is empty) and is not a candidate.
__global__ __launch_bounds__(DRAFT_T) void ngram_draft_kernel(const long* __restrict__ history, int hist_cap,
                                                              const int* __restrict__ hist_len, const long* __restrict__ cur,
                                                              const int* __restrict__ pos, const int* __restrict__ finished, int k,
                                                              int max_ngram, long pad, int* __restrict__ n_draft,
                                                              long* __restrict__ cur_rows, int* __restrict__ pos_rows) {
  __shared__ int s_best;
  const int s = blockIdx.x, tid = threadIdx.x, T = k + 1;
  const long* h = history + (long)s * hist_cap;
  const int len = min(max(hist_len[s], 0), hist_cap);
  int nd = 0, start = 0;
  if (finished[s] == 0) {  // (uniform)
    for (int n = min(max_ngram, len - 1); n >= 1; --n) {
      if (tid == 0) s_best = 0x7fffffff;
      __syncthreads();
      for (int i = tid; i < len - n; i += DRAFT_T) {
        bool match = true;
        for (int e = 0; e < n; ++e) match = match && h[i + e] == h[len - n + e];
        if (match) {  // (a thread's windows come in ascending order: its first match is its earliest)
          atomicMin(&s_best, i);
          break;
        }
      }
      __syncthreads();
      const int best = s_best;
      __syncthreads();  // (everyone has read s_best before the next round resets it)
      if (best != 0x7fffffff) {  // (uniform)
        start = best + n;
        nd = min(k, len - start);
        break;
      }
    }
  }
  if (tid < T) {
    cur_rows[(long)s * T + tid] = tid == 0 ? cur[s] : (tid <= nd ? h[start + tid - 1] : pad);
    pos_rows[(long)s * T + tid] = pos[s] + tid;
  }
  if (tid == 0) n_draft[s] = nd;
}

// Pass j of the verification: which logits row the sampler runs next.  Row s * T + j gets slot s when sequence s is still accepting
// -- pass 0: always (a finished sequence is inert in the sampler, as in the plain loop); pass j >= 1: every earlier pass accepted,
// draft j - 1 exists, the token selected by pass j - 1 (cur[s]) equals it and did not end the row (EOS, stop set, budget) -- and every
// other row gets -1.  One thread per row; a sequence's words (alive, drafted, accepted) are written by the thread of its row j only.
__global__ __launch_bounds__(256) void spec_gate_kernel(int j, int S, int T, const int* __restrict__ n_draft,
                                                        const long* __restrict__ cur_rows, const long* __restrict__ cur,
                                                        const int* __restrict__ finished, int* __restrict__ slot_of_row,
                                                        int* __restrict__ alive, int* __restrict__ drafted, int* __restrict__ accepted) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= S * T) return;
  const int s = r / T;
  if (r - s * T != j) {
    slot_of_row[r] = -1;
    return;
  }
  int a;
  if (j == 0) {
    a = 1;
    if (finished[s] == 0) drafted[s] += n_draft[s];
  } else {
    a = alive[s] != 0 && j <= n_draft[s] && finished[s] == 0 && cur[s] == cur_rows[r];
    if (a) accepted[s] += 1;
  }
  alive[s] = a;
  slot_of_row[r] = a ? s : -1;
}

}  // namespace tcavt

using namespace tcavt;

extern "C" int tcavt_ngram_draft(const int64_t* history, int hist_cap, const int32_t* hist_len, const int64_t* cur, const int32_t* pos,
                                 const int32_t* finished, int S, int k, int max_matching_ngram_size, int64_t pad_token_id,
                                 int32_t* n_draft, int64_t* cur_rows, int32_t* pos_rows, tcavt_stream_t stream) {
  const struct { const void* p; const char* name; } ptrs[] = {
      {history, "history"}, {hist_len, "hist_len"}, {cur, "cur"}, {pos, "pos"}, {finished, "finished"}, {n_draft, "n_draft"},
      {cur_rows, "cur_rows"}, {pos_rows, "pos_rows"}};
  for (const auto& a : ptrs) TCAVT_CHECK_ARG(a.p, "ngram_draft: %s is a null pointer", a.name);
  TCAVT_CHECK_ARG(S > 0, "ngram_draft: S = %d must be > 0", S);
  TCAVT_CHECK_ARG(hist_cap > 0, "ngram_draft: hist_cap = %d must be > 0", hist_cap);
  TCAVT_CHECK_ARG(k >= 1 && k < DRAFT_T, "ngram_draft: k = %d must be in [1, %d]", k, DRAFT_T - 1);
  TCAVT_CHECK_ARG(max_matching_ngram_size >= 1, "ngram_draft: max_matching_ngram_size = %d must be >= 1", max_matching_ngram_size);
  hipLaunchKernelGGL(ngram_draft_kernel, dim3(S), dim3(DRAFT_T), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const long*>(history), hist_cap, hist_len, reinterpret_cast<const long*>(cur), pos, finished, k,
                     max_matching_ngram_size, (long)pad_token_id, n_draft, reinterpret_cast<long*>(cur_rows), pos_rows);
  TCAVT_CHECK_LAUNCH("ngram_draft");
  return TCAVT_OK;
}

// T passes of (gate, tcavt_sample_tokens in its rows form): the selection, the ending rules and every state update are the plain
// sampler's own launches, on exactly the state the plain loop has at that token.
extern "C" int tcavt_spec_verify(const tcavt_spec_verify_args* a, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(a, "spec_verify: args is a null pointer");
  TCAVT_CHECK_ARG(a->sample, "spec_verify: sample is a null pointer");
  const struct { const void* p; const char* name; } ptrs[] = {
      {a->n_draft, "n_draft"}, {a->cur_rows, "cur_rows"}, {a->slot_of_row, "slot_of_row"}, {a->drafted, "drafted"},
      {a->accepted, "accepted"}, {a->sample->logits, "sample.logits"}, {a->sample->history, "sample.history"},
      {a->sample->hist_len, "sample.hist_len"}, {a->sample->params, "sample.params"}, {a->sample->step, "sample.step"},
      {a->sample->max_new, "sample.max_new"}, {a->sample->out_row, "sample.out_row"}, {a->sample->cur_tok, "sample.cur_tok"},
      {a->sample->pos, "sample.pos"}, {a->sample->finished, "sample.finished"}, {a->sample->out_tokens, "sample.out_tokens"}};
  for (const auto& q : ptrs) TCAVT_CHECK_ARG(q.p, "spec_verify: %s is a null pointer", q.name);
  TCAVT_CHECK_ARG(a->S > 0, "spec_verify: S = %d must be > 0", a->S);
  TCAVT_CHECK_ARG(a->T >= 1 && a->T <= 256, "spec_verify: T = %d must be in [1, 256]", a->T);
  TCAVT_CHECK_ARG((long)a->S * a->T <= (1L << 20), "spec_verify: S * T too large");
  TCAVT_CHECK_ARG(a->sample->V > 0 && a->sample->hist_cap > 0 && a->sample->out_cap > 0,
                  "spec_verify: sample.V, sample.hist_cap and sample.out_cap must be > 0");
  const tcavt_sample_params* sp = a->sample->params;
  TCAVT_CHECK_ARG(!sp->do_sample || (sp->temperature > 0.f && sp->top_k >= 1 && sp->top_p > 0.f && sp->top_p <= 1.f),
                  "spec_verify: sampling needs temperature > 0, top_k >= 1, 0 < top_p <= 1");
  TCAVT_CHECK_ARG(sp->repetition_penalty > 0.f && sp->no_repeat_ngram_size >= 0, "spec_verify: bad repetition_penalty / no_repeat_ngram_size");
  const int R = a->S * a->T;
  tcavt_sample_args sa = *a->sample;
  sa.slot_of_row = a->slot_of_row;
  sa.rows = R;
  sa.n_state = a->S;
  for (int j = 0; j < a->T; ++j) {
    hipLaunchKernelGGL(spec_gate_kernel, dim3((R + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), j, a->S, a->T, a->n_draft,
                       reinterpret_cast<const long*>(a->cur_rows), reinterpret_cast<const long*>(sa.cur_tok), sa.finished, a->slot_of_row,
                       a->slot_of_row + R, a->drafted, a->accepted);
    TCAVT_CHECK_LAUNCH("spec_verify");
    const int rc = tcavt_sample_tokens(&sa, stream);
    if (rc != TCAVT_OK) return rc;
  }
  return TCAVT_OK;
}
