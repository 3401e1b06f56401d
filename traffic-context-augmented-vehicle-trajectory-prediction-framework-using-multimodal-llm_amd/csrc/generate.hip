// Autoregressive text generation on the decoder stack (reference: LlamaMultiModal.generate_batch,
// scripts/train.py:577-654, and scripts/check_generation.py:152-222).
//
// The reference hands HF `generate` a prefix of image tokens + prompt embeddings through a patched embedding layer and
// samples with temperature 0.9, top-k 40, top-p 0.9, repetition penalty 1.2 and no-repeat-3-grams (train.py:628-642).
// Here the prefix is a first-class argument: the PREFILL is the ordinary batched forward (tcavt_llama_stack_forward
// with k_cache / v_cache set), and every following token is ONE call of tcavt_llama_decode_step:
//
//   embed (table[id] + text modality embedding)  ->  16 x [ LoRA down | q|k|v + RoPE at the sample's own position |
//   attention of the one query over the cached keys (which also appends the new k, v) | o_proj | gate|up | down ]  ->
//   final RMSNorm  ->  lm_head (tied embedding table)  ->  logits processors + token selection (tcavt_sample_logits)
//
// All per-step state (positions, current tokens, token history, step counter, finished flags) lives on the device and
// is advanced by the selection kernel, so the launch sequence of a step never changes: it is captured in a hipGraph
// once and replayed per token (BASELINE.json configs[4] "hipGraph-captured decode").
// The projections reuse the MFMA GEMM (M = batch rows: weight-streaming, HBM-bound); RMSNorm is fused exactly as in the
// prefill (csrc/stack.hip).  This file is the step itself; its attention is csrc/attn_decode.hip (attn_decode_shared.hip), the
// selection csrc/sampler.hip, and the kernels that move a prefilled cache into a decode batch csrc/kv_move.hip.
// tcavt_llama_decode_step_multi is the same step on T consecutive positions per sequence (prompt-lookup speculative decoding: the
// draft and the verification around it are csrc/spec.hip).
#include "common.hpp"

namespace tcavt {

// out[b] = src[b * L + kv_len[b] - 1]  (the last valid position's hidden state of each sample after the prefill)
__global__ __launch_bounds__(256) void gather_last_kernel(const bf16_t* __restrict__ src, const int* __restrict__ kv_len,
                                                          bf16_t* __restrict__ out, int L, int H) {
  const int b = blockIdx.x;
  const int l = min(max(kv_len[b], 1), L) - 1;
  const bf16_t* s = src + ((long)b * L + l) * H;
  for (int c = threadIdx.x * 8; c < H; c += 256 * 8)
    *reinterpret_cast<u32x4*>(out + (long)b * H + c) = *reinterpret_cast<const u32x4*>(s + c);
}

}  // namespace tcavt

using namespace tcavt;

#define TCAVT_TRY(call)              \
  do {                               \
    const int rc_ = (call);          \
    if (rc_ != TCAVT_OK) return rc_; \
  } while (0)

extern "C" int tcavt_gather_last(const void* src16, const int32_t* kv_len, void* out16, int B, int L, int H,
                                 tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(src16 && kv_len && out16 && B > 0 && L > 0 && H > 0 && H % 8 == 0, "gather_last: bad args");
  hipLaunchKernelGGL(gather_last_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(src16), kv_len, static_cast<bf16_t*>(out16), L, H);
  TCAVT_CHECK_LAUNCH("gather_last");
  return TCAVT_OK;
}

// The decode step; px != NULL: the rows read their prompts' cache in place (tcavt_llama_decode_step_shared); T > 0: the B rows are
// T consecutive positions of each of B / T sequences on one cache per sequence (tcavt_llama_decode_step_multi).
static int decode_step_impl(const tcavt_decode_args* a, const tcavt_kv_prefix* px, tcavt_stream_t stream, int T = 0) {
  TCAVT_CHECK_ARG(a && a->layers && a->gamma_final && a->rope_cos && a->rope_sin && a->table && a->txt_mod && a->cur_tok && a->pos &&
                      a->h16 && a->part && a->qkv && a->att && a->act && a->x16 && a->logits && a->bad_id_flag,
                  "llama_decode_step: null pointer");
  // the cache: the 16-bit pair, or the four FP8 planes (tcavt_attn_decode8) -- one of the two
  const bool kv8 = a->kv8_k_codes || a->kv8_k_scales || a->kv8_v_codes || a->kv8_v_scales;
  TCAVT_CHECK_ARG(!kv8 || (a->kv8_k_codes && a->kv8_k_scales && a->kv8_v_codes && a->kv8_v_scales),
                  "llama_decode_step: the four kv8 planes come together");
  TCAVT_CHECK_ARG(!kv8 || (!a->k_cache && !a->v_cache), "llama_decode_step: the kv8 planes and k_cache / v_cache exclude each other");
  TCAVT_CHECK_ARG(kv8 || (a->k_cache && a->v_cache), "llama_decode_step: null pointer (k_cache / v_cache, or the four kv8 planes)");
  if (T > 0) {
    TCAVT_CHECK_ARG(!kv8, "llama_decode_step_multi: the kv8 planes are not supported");
    TCAVT_CHECK_ARG(a->B > 0 && a->B % T == 0, "llama_decode_step_multi: B = %d must be a multiple of T = %d", a->B, T);
    TCAVT_CHECK_ARG(a->B <= 32, "llama_decode_step_multi: B = %d rows exceed 32", a->B);
    TCAVT_CHECK_ARG(T <= a->kv_lmax, "llama_decode_step_multi: T = %d exceeds kv_lmax = %d", T, a->kv_lmax);
    TCAVT_CHECK_ARG(a->rope_L >= a->kv_lmax, "llama_decode_step_multi: rope_L = %d must be >= kv_lmax = %d", a->rope_L, a->kv_lmax);
  }
  // the shared prompt cache (tcavt_attn_decode_shared): k_cache / v_cache then hold the rows' suffixes only
  if (px) {
    TCAVT_CHECK_ARG(!kv8, "llama_decode_step: prefix and the kv8 planes exclude each other");
    TCAVT_CHECK_ARG(px->k && px->v && px->len, "llama_decode_step: prefix: null pointer (k, v, len)");
    TCAVT_CHECK_ARG(px->n >= 1 && px->lmax >= 1, "llama_decode_step: prefix: n = %d and lmax = %d must be >= 1", px->n, px->lmax);
    TCAVT_CHECK_ARG(a->B > 0 && a->B % px->n == 0, "llama_decode_step: prefix: B = %d must be a multiple of n = %d", a->B, px->n);
    TCAVT_CHECK_ARG((long)a->rope_L >= (long)px->lmax + a->kv_lmax, "llama_decode_step: prefix: rope_L = %d must be >= lmax + kv_lmax = %ld",
                    a->rope_L, (long)px->lmax + a->kv_lmax);
    TCAVT_CHECK_ARG(a->kv_lmax <= TCAVT_ATTN_DECODE_SHARED_MAX_SUFFIX,
                    "llama_decode_step: prefix: kv_lmax = %d exceeds TCAVT_ATTN_DECODE_SHARED_MAX_SUFFIX = %d", a->kv_lmax,
                    TCAVT_ATTN_DECODE_SHARED_MAX_SUFFIX);
  }
  TCAVT_CHECK_ARG(a->n_layers > 0 && a->B > 0 && a->H % 256 == 0 && a->I > 0 && a->nq > 0 && a->nkv > 0 && a->nq % a->nkv == 0 &&
                      a->nq / a->nkv <= 8 && a->V > 0 && a->V % 16 == 0 && a->kv_lmax > 0 && a->rope_L >= a->kv_lmax && is16(a->dtype16),
                  "llama_decode_step: bad shape (H %% 256, V %% 16, nq / nkv <= 8, rope_L >= kv_lmax)");
  const int B = a->B, H = a->H, I = a->I, nq = a->nq, nkv = a->nkv, dt = a->dtype16;
  const int nqkv = (nq + 2 * nkv) * 64;
  const int np_in = norm_out_npart(B, H, I), np_post = norm_out_npart(B, H, nq * 64);  // see csrc/stack.hip
  // scaled 16-bit image of the residual stream, as in tcavt_llama_stack_forward (the prefill that filled the cache ran at the same scale
  // or not: keys / values are true-scale either way)
  TCAVT_CHECK_ARG(a->stream_scale >= 0.f && a->stream_scale <= 1.f, "llama_decode_step: stream_scale must be in (0, 1] (0 means 1)");
  const float ss_ = a->stream_scale == 0.f ? 1.f : a->stream_scale;
  const float eps_s = a->rms_eps * ss_ * ss_;
  // fragment-major weight copies (tcavt_pack_weight16): the projections' weight streams read consecutive bytes; or their FP8
  // form (tcavt_pack_weight8): half the bytes
  const int wl = a->w_layout;
  TCAVT_CHECK_ARG(wl == 0 || ((wl == TCAVT_W_FRAG16 || wl == TCAVT_W_FRAG8) && B <= 32 && I % 256 == 0 && (nq * 64) % 256 == 0),
                  "llama_decode_step: w_layout must be 0, TCAVT_W_FRAG16 or TCAVT_W_FRAG8 (B <= 32, I %% 256 == 0, nq * 64 %% 256 == 0)");
  TCAVT_CHECK_ARG(wl != TCAVT_W_FRAG8 || a->table_packed, "llama_decode_step: TCAVT_W_FRAG8 needs table_packed (the tcavt_pack_weight8 copy of table)");
  // fragment-major activations: h16, att, act, x16 in the skinny GEMMs' operand order (16 or 32 whole rows each)
  const int al = a->act_layout;
  TCAVT_CHECK_ARG(al == 0 || ((al == 1 || al == 2) && a->h == nullptr && B <= (al == 2 ? 8 : 32) && I % 256 == 0 && (nq * 64) % 256 == 0),
                  "llama_decode_step: act_layout must be 0, 1 (B <= 32) or 2 (B <= 8) (16-bit residual stream: h == NULL; I %% 256 == 0, "
                  "nq * 64 %% 256 == 0)");
  const int blk8 = al == 2 ? TCAVT_ACT_BLOCK8 : 0;
  const int gA = al ? (TCAVT_ACT_A_FRAG16 | blk8) : 0, gAO = al ? (TCAVT_ACT_A_FRAG16 | TCAVT_ACT_OUT_FRAG16 | blk8) : 0;
  // h = table[cur_tok] + text modality embedding (generated tokens are text tokens: scripts/train.py:526-527); + the fused
  // norm's inputs
  // (a->h == NULL: the residual stream is the 16-bit h16 itself, as in tcavt_llama_stack_forward)
  TCAVT_TRY(embed_fuse_impl(a->table, a->cur_tok, a->txt_mod /* unused: Nq = 0 */, a->txt_mod, a->txt_mod, a->h, B, 0, 1, H, a->V,
                            a->bad_id_flag, dt, a->h16, a->part, np_in, ss_, al, stream));
  const size_t per_layer = (size_t)(T > 0 ? B / T : B) * a->kv_lmax * nkv * 64;
  {
    int KS;
    size_t lds;
    TCAVT_CHECK_ARG(attn_decode_rule(a->kv_lmax, &KS, &lds), "llama_decode_step: kv_lmax = %d too long for the decode attention's score buffer",
                    a->kv_lmax);
  }
  for (int li = 0; li < a->n_layers; ++li) {
    const tcavt_llama_layer& w = a->layers[li];
    TCAVT_CHECK_ARG(w.w_qkv && w.w_o && w.w_gu && w.w_d && (!w.a_cat || (w.b_ext && a->t)), "llama_decode_step: layer %d: null weight", li);
    // LoRA down-projection: a launch of its own for layer 0 (and without a->lora_part); layers 1.. read the partial sums the
    // previous layer's down-projection GEMM wrote next to its residual epilogue
    // (a q|k|v workgroup reads the partial sums of its own tokens: all B for B <= 16, its 16-token block beyond)
    const bool lp_ok = a->lora_part && a->lora_rank > 0 && a->lora_rank <= 8 && B <= 32;
    const bool t_fused = lp_ok && li > 0 && w.a_cat && a->layers[li - 1].w_d;
    if (w.a_cat && !t_fused) {
      tcavt_gemm_args g = {};
      g.A = a->h16; g.lda = H; g.W = w.a_cat; g.ldw = H; g.C = a->t; g.ldc = 64; g.M = B; g.N = 64; g.K = H; g.act_layout = gA;
      g.out_dtype = dt; g.in_dtype = dt; g.acc_scale = a->lora_scale;  // (t is at the stream's scale, like the main term of the accumulator)
      g.splitk_ws = a->splitk_ws; g.splitk_ws_bytes = a->splitk_ws_bytes;
      TCAVT_TRY(tcavt_gemm_bf16(&g, stream));
    }
    {
      tcavt_gemm_args g = {};
      g.A = a->h16; g.lda = H; g.W = w.w_qkv; g.ldw = H; g.C = a->qkv; g.ldc = nqkv; g.w_layout = wl; g.act_layout = gA;
      g.M = B; g.N = nqkv; g.K = H; g.out_dtype = dt; g.in_dtype = dt;
      if (t_fused) {
        g.W2 = w.b_ext; g.ldw2 = 64; g.lora_part = a->lora_part; g.lora_part_np = H / 16; g.lora_part_scale = a->lora_scale;
      } else if (w.a_cat) { g.A2 = a->t; g.lda2 = 64; g.W2 = w.b_ext; g.ldw2 = 64; g.K2 = 64; }
      g.epilogue = TCAVT_EPI_ROPE | TCAVT_EPI_ROWSCALE;
      g.rope_cos = a->rope_cos; g.rope_sin = a->rope_sin; g.rope_L = a->rope_L; g.rope_cols = (nq + nkv) * 64;
      g.rope_pos = a->pos;
      g.rowscale_part = a->part; g.rowscale_npart = np_in; g.rowscale_h = H; g.rowscale_eps = eps_s;
      g.splitk_ws = a->splitk_ws; g.splitk_ws_bytes = a->splitk_ws_bytes;
      TCAVT_TRY(tcavt_gemm_bf16(&g, stream));
    }
    // (the new token's k / v rows are appended to the cache by the attention kernel itself)
    if (kv8) {
      const size_t rows = (size_t)li * B * nkv * a->kv_lmax;  // cached rows in front of this layer's planes
      TCAVT_TRY(tcavt_attn_decode8(a->qkv, static_cast<unsigned char*>(a->kv8_k_codes) + rows * 64, static_cast<unsigned char*>(a->kv8_k_scales) + rows * 2,
                                   static_cast<unsigned char*>(a->kv8_v_codes) + rows * 64, static_cast<unsigned char*>(a->kv8_v_scales) + rows * 2,
                                   a->pos, a->att, B, nq, nkv, a->kv_lmax, 0.125f, dt, al, stream));
    } else if (px) {
      const size_t pre_layer = (size_t)(B / px->n) * px->lmax * nkv * 64;
      TCAVT_TRY(tcavt_attn_decode_shared(a->qkv, static_cast<const bf16_t*>(px->k) + li * pre_layer, static_cast<const bf16_t*>(px->v) + li * pre_layer,
                                         px->len, static_cast<bf16_t*>(a->k_cache) + li * per_layer, static_cast<bf16_t*>(a->v_cache) + li * per_layer,
                                         a->pos, a->att, B / px->n, px->n, nq, nkv, px->lmax, a->kv_lmax, 0.125f, dt, al, stream));
    } else {
      bf16_t* kc = static_cast<bf16_t*>(a->k_cache) + li * per_layer;
      bf16_t* vc = static_cast<bf16_t*>(a->v_cache) + li * per_layer;
      if (T > 0) TCAVT_TRY(tcavt_attn_decode_multi(a->qkv, kc, vc, a->pos, a->att, B / T, T, nq, nkv, a->kv_lmax, 0.125f, dt, al, stream));
      else TCAVT_TRY(tcavt_attn_decode(a->qkv, kc, vc, a->pos, a->att, B, nq, nkv, a->kv_lmax, 0.125f, dt, al, stream));
    }
    {
      tcavt_gemm_args g = {};
      g.A = a->att; g.lda = nq * 64; g.W = w.w_o; g.ldw = nq * 64; g.C = a->h; g.ldc = H; g.w_layout = wl; g.act_layout = gAO;
      g.M = B; g.N = H; g.K = nq * 64; g.out_dtype = TCAVT_F32; g.in_dtype = dt;
      g.residual = a->h; g.ldr = H; g.epilogue = TCAVT_EPI_RESIDUAL | TCAVT_EPI_NORM_OUT;
      g.norm_h16 = a->h16; g.norm_part = a->part; g.norm_scale = ss_;
      g.nonfinite_flag = a->nonfinite_flag; g.nonfinite_tag = 1 + 2 * li;
      g.splitk_ws = a->splitk_ws; g.splitk_ws_bytes = a->splitk_ws_bytes;
      TCAVT_TRY(tcavt_gemm_bf16(&g, stream));
    }
    {
      tcavt_gemm_args g = {};
      g.A = a->h16; g.lda = H; g.W = w.w_gu; g.ldw = H; g.C = a->act; g.ldc = I; g.w_layout = wl; g.act_layout = gAO;
      g.M = B; g.N = 2 * I; g.K = H; g.out_dtype = dt; g.in_dtype = dt;
      g.epilogue = TCAVT_EPI_SILU_MUL | TCAVT_EPI_ROWSCALE;
      g.rowscale_part = a->part; g.rowscale_npart = np_post; g.rowscale_h = H; g.rowscale_eps = eps_s;
      g.splitk_ws = a->splitk_ws; g.splitk_ws_bytes = a->splitk_ws_bytes;
      TCAVT_TRY(tcavt_gemm_bf16(&g, stream));
    }
    {
      tcavt_gemm_args g = {};
      g.A = a->act; g.lda = I; g.W = w.w_d; g.ldw = I; g.C = a->h; g.ldc = H; g.w_layout = wl; g.act_layout = gAO;
      g.M = B; g.N = H; g.K = I; g.out_dtype = TCAVT_F32; g.in_dtype = dt;
      g.residual = a->h; g.ldr = H; g.epilogue = TCAVT_EPI_RESIDUAL | TCAVT_EPI_NORM_OUT;
      g.norm_h16 = a->h16; g.norm_part = a->part; g.norm_scale = ss_;
      g.nonfinite_flag = a->nonfinite_flag; g.nonfinite_tag = 2 + 2 * li;
      if (lp_ok && li + 1 < a->n_layers && a->layers[li + 1].a_cat) {
        g.lora_part = a->lora_part; g.lora_part_a = a->layers[li + 1].a_cat; g.lora_part_lda = H;
      }
      g.splitk_ws = a->splitk_ws; g.splitk_ws_bytes = a->splitk_ws_bytes;
      TCAVT_TRY(tcavt_gemm_bf16(&g, stream));
    }
  }
  if (a->h == nullptr) TCAVT_TRY(rmsnorm16_impl(a->h16, a->gamma_final, eps_s, a->x16, nullptr, B, H, dt, al, stream));
  else TCAVT_TRY(tcavt_rmsnorm(a->h, a->gamma_final, a->rms_eps, a->x16, nullptr, B, H, nullptr, 0.f, 0, 0, dt, stream));
  // lm_head: tied to the embedding table (Llama-3.2-1B: tie_word_embeddings)
  tcavt_gemm_args g = {};
  g.A = a->x16; g.lda = H; g.W = a->table; g.ldw = H; g.C = a->logits; g.ldc = a->V;
  if (a->table_packed && B <= 32) { g.W = a->table_packed; g.w_layout = wl == TCAVT_W_FRAG8 ? TCAVT_W_FRAG8 : TCAVT_W_FRAG16; }
  g.act_layout = gA;
  g.M = B; g.N = a->V; g.K = H; g.out_dtype = TCAVT_F32; g.in_dtype = dt;
  g.splitk_ws = a->splitk_ws; g.splitk_ws_bytes = a->splitk_ws_bytes;
  return tcavt_gemm_bf16(&g, stream);
}

extern "C" int tcavt_llama_decode_step(const tcavt_decode_args* a, tcavt_stream_t stream) { return decode_step_impl(a, nullptr, stream); }

extern "C" int tcavt_llama_decode_step_shared(const tcavt_decode_args* a, const tcavt_kv_prefix* prefix, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(prefix, "llama_decode_step_shared: prefix is a null pointer");
  return decode_step_impl(a, prefix, stream);
}

extern "C" int tcavt_llama_decode_step_multi(const tcavt_decode_args* a, int T, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(a, "llama_decode_step_multi: args is a null pointer");
  TCAVT_CHECK_ARG(T >= 1, "llama_decode_step_multi: T = %d must be >= 1", T);
  return decode_step_impl(a, nullptr, stream, T);
}
